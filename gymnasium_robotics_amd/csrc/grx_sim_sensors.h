// grx_sim_sensors.h -- MjData.sensordata of the task-free stepper for the MJCF's <sensor> children other than touch and rangefinder: joint, actuator, frame and IMU readings
// (include/grx_capi.h grx_sim_sensors).  Plain lane code over GrxCtx: the lane emulator compiles this header too (tests/emu/grx_emu_sensors.cpp).
//
// All readings belong to ONE forward pass, in two phases around its solve, because the acceleration types need both halves of
//   c     = Jp a + (d/dt Jp) v      (the classical acceleration of the material point p of the object)
//   alpha = Jr a + (d/dt Jr) v
// and the two halves never exist together: (d/dt J) v is made from cvel and cdof_dot, which live in the P1 overlay the solve reuses (grx_ctx_carve), a exists after the solve.
//   phase 1, between grx_velocity and grx_solve_integrate: every position, velocity, joint and actuator reading, complete; of the acceleration types the part without a:
//            sum_chain cdof_dot[d] qvel[d] shifted to p, the centripetal correction omega x u, and -g (MuJoCo's convention: cacc of the world body is -gravity, so an
//            accelerometer at rest reads +|g| along world z).  The partial goes into the world's own output row: no LDS is added and there is no sensor limit.
//   phase 2, after the solve: the lane that wrote the partial adds sum_chain cdof[d] qacc[d] shifted to p (cdof, xpos, sxpos are persistent), rotates into the site frame
//            where the type asks for it, and clamps to the cutoff.
// Sensor s is served by lane s mod 64 in both phases, so a lane reads back only what it wrote itself.
//
// THE FREE JOINT.  The generic engine leaves a free joint's three linear dofs out of cvel and zeroes their cdof_dot (grx_eng_velocity.h, flinmask): it watches the tree from a
// frame that moves with that constant velocity.  Accelerations are the same in both frames, velocities are not:
//   * velocimeter / framelinvel walk the dof chain with cdof and the full qvel (GrxFetch<S>::grx_point_velocity), never cvel;
//   * the omega x u term uses u of the REDUCED velocity (cvel), the one cdof_dot was built with: in that frame c = a_spatial(p) + omega x u holds as it stands.
#pragma once
#include "grx_engine.h"
#include "grx_fetch_task.h"   // GrxFetch<S>::grx_point_velocity

// sensor types (spec[4 s]) and object types (spec[4 s + 1]); the host table of grx_sim_step_sns names them with these numbers (gymnasium_robotics_amd/sim.py SENSOR_TYPES)
enum { GRX_SNS_JOINTPOS = 0, GRX_SNS_JOINTVEL, GRX_SNS_ACTUATORPOS, GRX_SNS_ACTUATORVEL, GRX_SNS_ACTUATORFRC, GRX_SNS_JOINTACTFRC, GRX_SNS_FRAMEPOS, GRX_SNS_FRAMEQUAT,
       GRX_SNS_FRAMEXAXIS, GRX_SNS_FRAMEYAXIS, GRX_SNS_FRAMEZAXIS, GRX_SNS_FRAMELINVEL, GRX_SNS_FRAMEANGVEL, GRX_SNS_VELOCIMETER, GRX_SNS_GYRO, GRX_SNS_FRAMELINACC,
       GRX_SNS_FRAMEANGACC, GRX_SNS_ACCELEROMETER, GRX_SNS_NTYPE };
enum { GRX_SNS_OBJ_JOINT = 0, GRX_SNS_OBJ_ACTUATOR, GRX_SNS_OBJ_SITE, GRX_SNS_OBJ_XBODY, GRX_SNS_NOBJ };

// The fifth optional block as the kernels see it: spec and cutoff are the handle's DEVICE copies of the caller's host tables (grx_sim_step_sns swaps them in).
struct GrxSimSensors {
  const int* spec;       // [nsensor,4] = type, objtype, objid, adr
  const float* cutoff;   // [nsensor]; > 0 clamps the reading to [-cutoff, cutoff] (not the quaternion and axis types)
  int nsensor, ndata;
  float* data;           // [N,ndata]
};

GRX_HD int grx_sensor_dim(int type) { return type == GRX_SNS_FRAMEQUAT ? 4 : (type >= GRX_SNS_FRAMEPOS ? 3 : 1); }
GRX_HD int grx_sensor_is_acc(int type) { return type >= GRX_SNS_FRAMELINACC; }

template <class S>
struct GrxSns {
  // the object's body, position and rotation (row-major, local -> world) in the pass's kinematics
  GRX_MEM void grx_sensor_object(const GrxModel* m, const GrxCtx* c, int objtype, int id, int& b, const float*& p, const float*& R) {
    if (objtype == GRX_SNS_OBJ_SITE) { b = m->site_bodyid[id]; p = c->sxpos + 3 * id; R = c->sxmat + 9 * id; }
    else { b = id; p = c->xpos + 3 * id; R = c->xmat + 9 * id; }
  }
  // mju_mat2Quat: the unit quaternion (w, x, y, z) of a rotation matrix, from its largest diagonal combination
  GRX_MEM void grx_sensor_mat2quat(const float* R, float* q) {
    const float tr = R[0] + R[4] + R[8];
    if (tr > 0.0f) { q[0] = 0.5f * sqrtf(1.0f + tr); const float s = 0.25f / q[0]; q[1] = s * (R[7] - R[5]); q[2] = s * (R[2] - R[6]); q[3] = s * (R[3] - R[1]); }
    else if (R[0] > R[4] && R[0] > R[8]) { q[1] = 0.5f * sqrtf(1.0f + R[0] - R[4] - R[8]); const float s = 0.25f / q[1]; q[0] = s * (R[7] - R[5]); q[2] = s * (R[1] + R[3]); q[3] = s * (R[2] + R[6]); }
    else if (R[4] > R[8]) { q[2] = 0.5f * sqrtf(1.0f - R[0] + R[4] - R[8]); const float s = 0.25f / q[2]; q[0] = s * (R[2] - R[6]); q[1] = s * (R[1] + R[3]); q[3] = s * (R[5] + R[7]); }
    else { q[3] = 0.5f * sqrtf(1.0f - R[0] - R[4] + R[8]); const float s = 0.25f / q[3]; q[0] = s * (R[3] - R[1]); q[1] = s * (R[2] + R[6]); q[2] = s * (R[5] + R[7]); }
    const float n = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; k++) q[k] *= n;
  }
  // the actuator's scalar force before the gear: gain * clamp(ctrl) + bias, clamped to forcerange -- grx_actuator_force (csrc/grx_eng_velocity.h) without its final multiply
  GRX_MEM float grx_sensor_actuator_force(const GrxModel* m, const GrxCtx* c, int i) {
    const int* AI = m->reci_act + GRX_RAI * i; const float* AF = m->recf_act + GRX_RAF * i;
    const float gear = AF[0];
    const float len = gear * c->qpos[AI[0]], vel = gear * c->qvel[AI[1]];
    float u = c->ctrl[i];
    if (AI[2]) u = fminf(AF[2], fmaxf(AF[1], u));
    float gain = AF[3];
    if (AI[3] == 1) gain += AF[4] * len + AF[5] * vel;
    float bias = 0;
    if (AI[4] == 1) bias = AF[6] + AF[7] * len + AF[8] * vel;
    float f = gain * u + bias;
    if (AI[5]) f = fminf(AF[10], fmaxf(AF[9], f));
    return f;
  }
  GRX_MEM float grx_sensor_clamp(float v, float cut) { return cut > 0.0f ? fminf(cut, fmaxf(-cut, v)) : v; }

  // Phase 1 (header).  row: this world's [ndata] output row.  Needs the pass's own qpos, qvel, ctrl, cvel, cdof_dot and qfrc_actuator: call it between grx_velocity and the solve.
  GRX_MEM void grx_sim_sensors_p1(const GrxModel* m, const GrxCtx* c, const GrxSimSensors* sn, float* row, int lane_) {
    GRX_FRESH_MODEL(m, c);
    const int ns = sn->nsensor;
    FOR_LANES {
      for (int s = lane; s < ns; s += 64) {
        const int* sp = sn->spec + 4 * s;
        const int type = sp[0], objtype = sp[1], id = sp[2], adr = sp[3];
        const float cut = sn->cutoff[s];
        float out[4] = {0, 0, 0, 0};
        if (type <= GRX_SNS_JOINTACTFRC) {
          if (type == GRX_SNS_JOINTPOS) out[0] = c->qpos[m->jnt_qposadr[id]];
          else if (type == GRX_SNS_JOINTVEL) out[0] = c->qvel[m->jnt_dofadr[id]];
          else if (type == GRX_SNS_JOINTACTFRC) out[0] = c->qfrc_actuator[m->jnt_dofadr[id]];
          else if (type == GRX_SNS_ACTUATORFRC) out[0] = grx_sensor_actuator_force(m, c, id);
          else {
            const int* AI = m->reci_act + GRX_RAI * id; const float gear = m->recf_act[GRX_RAF * id];
            out[0] = type == GRX_SNS_ACTUATORPOS ? gear * c->qpos[AI[0]] : gear * c->qvel[AI[1]];
          }
          row[adr] = grx_sensor_clamp(out[0], cut);
          continue;
        }
        int b; const float *p, *R;
        grx_sensor_object(m, c, objtype, id, b, p, R);
        if (type == GRX_SNS_FRAMEPOS) { for (int k = 0; k < 3; k++) row[adr + k] = grx_sensor_clamp(p[k], cut); }
        else if (type == GRX_SNS_FRAMEQUAT) { grx_sensor_mat2quat(R, out); for (int k = 0; k < 4; k++) row[adr + k] = out[k]; }
        else if (type <= GRX_SNS_FRAMEZAXIS) { const int col = type - GRX_SNS_FRAMEXAXIS; for (int k = 0; k < 3; k++) row[adr + k] = R[3 * k + col]; }
        else if (type <= GRX_SNS_GYRO) {
          float vp[3], vr[3];
          GrxFetch<S>::grx_point_velocity(m, c, b, p, vp, vr);   // the dof chain with the FULL qvel: a free joint's linear dofs included
          const float* v = (type == GRX_SNS_FRAMELINVEL || type == GRX_SNS_VELOCIMETER) ? vp : vr;
          const int local = (type == GRX_SNS_VELOCIMETER || type == GRX_SNS_GYRO);
          for (int k = 0; k < 3; k++) {
            const float x = local ? R[k] * v[0] + R[3 + k] * v[1] + R[6 + k] * v[2] : v[k];   // R' v
            row[adr + k] = grx_sensor_clamp(x, cut);
          }
        } else {
          // the part of the acceleration that does not contain qacc: (d/dt J) v about the tree's reference point, shifted to p
          const float* cref = c->xpos + 3 * m->body_rootid[b];
          const float off[3] = {p[0] - cref[0], p[1] - cref[1], p[2] - cref[2]};
          float ab[6] = {0, 0, 0, 0, 0, 0};
          for (int d = m->body_lastdof[b]; d >= 0; d = m->dof_parentid[d]) {
            const float qd = c->qvel[d]; const float* cdd = c->cdof_dot + 6 * d;
            for (int k = 0; k < 6; k++) ab[k] += cdd[k] * qd;
          }
          if (type == GRX_SNS_FRAMEANGACC) { for (int k = 0; k < 3; k++) row[adr + k] = ab[k]; }
          else {
            const float* cv = c->cvel + 6 * b;   // the REDUCED velocity: what cdof_dot was built with
            float t[3], u[3], wu[3], sh[3];
            cross3f(t, cv, off);
            for (int k = 0; k < 3; k++) u[k] = cv[3 + k] + t[k];
            cross3f(wu, cv, u);      // omega x u: spatial -> classical acceleration
            cross3f(sh, ab, off);
            for (int k = 0; k < 3; k++) row[adr + k] = ab[3 + k] + sh[k] + wu[k] - m->gravity[k];
          }
        }
      }
    }
  }
  // Phase 2 (header): after the solve of the same pass.  Needs qacc and the persistent cdof, xpos, xmat, sxpos, sxmat.
  GRX_MEM void grx_sim_sensors_p2(const GrxModel* m, const GrxCtx* c, const GrxSimSensors* sn, float* row, int lane_) {
    GRX_FRESH_MODEL(m, c);
    const int ns = sn->nsensor;
    FOR_LANES {
      for (int s = lane; s < ns; s += 64) {
        const int* sp = sn->spec + 4 * s;
        const int type = sp[0], objtype = sp[1], id = sp[2], adr = sp[3];
        if (!grx_sensor_is_acc(type)) continue;
        const float cut = sn->cutoff[s];
        int b; const float *p, *R;
        grx_sensor_object(m, c, objtype, id, b, p, R);
        const float* cref = c->xpos + 3 * m->body_rootid[b];
        const float off[3] = {p[0] - cref[0], p[1] - cref[1], p[2] - cref[2]};
        float ja[6] = {0, 0, 0, 0, 0, 0};
        for (int d = m->body_lastdof[b]; d >= 0; d = m->dof_parentid[d]) {
          const float qa = c->qacc[d]; const float* cd = c->cdof + 6 * d;
          for (int k = 0; k < 6; k++) ja[k] += cd[k] * qa;
        }
        float v[3];
        if (type == GRX_SNS_FRAMEANGACC) { for (int k = 0; k < 3; k++) v[k] = row[adr + k] + ja[k]; }
        else {
          float sh[3]; cross3f(sh, ja, off);
          for (int k = 0; k < 3; k++) v[k] = row[adr + k] + ja[3 + k] + sh[k];
        }
        for (int k = 0; k < 3; k++) {
          const float x = type == GRX_SNS_ACCELEROMETER ? R[k] * v[0] + R[3 + k] * v[1] + R[6 + k] * v[2] : v[k];   // R' v
          row[adr + k] = grx_sensor_clamp(x, cut);
        }
      }
    }
  }
};
