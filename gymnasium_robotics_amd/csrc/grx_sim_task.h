// grx_sim_task.h -- the task-free stepper: mj_step(nstep) / mj_forward for a caller's own compiled model, and the MjData fields custom environments read afterwards.
//
// Device restatement of
//   MujocoRobotEnv._mujoco_step .... gymnasium_robotics/envs/robot_env.py:341  (mujoco.mj_step(model, data, nstep = n_substeps))
//   mujoco.mj_forward .............. envs/robot_env.py:300-313, envs/fetch/fetch_env.py:401     (after a state was written into MjData)
//   get_site_xpos / _xvelp / _xvelr  utils/mujoco_utils.py (data.site_xpos[id]; jacp @ data.qvel; jacr @ data.qvel)
// No action mapping, no observation, no reward: ctrl and the mocap poses are state the caller writes, the outputs are the derived fields of the LAST forward pass.
#pragma once
#include "grx_engine.h"
#include "grx_fetch_task.h"   // GrxFetch<S>::grx_point_velocity: J(site) * qvel from the motion axes of the last pass
#if defined(GRX_SIM_SENSORS)
#include "grx_sim_sensors.h"  // the fifth optional block (GrxSimSensors), only in the units compiled with GRX_SIM_SENSORS: every other unit compiles the lines it always compiled
#endif

struct GrxSimBuffers {
  float *qpos, *qvel, *qacc_ws;           // [N,nq] [N,nv] [N,nv]
  const float* ctrl;                      // [N,nu]
  const float *mocap_pos, *mocap_quat;    // [N,nmocap,3] [N,nmocap,4]
  float *xpos, *xquat, *site_xpos, *site_xmat, *site_xvelp, *site_xvelr, *sensordata;   // optional outputs (null: not written)
  int *ncon, *nefc;                       // [N] optional
  int* status;                            // [N]
  const unsigned char* mask;              // [N] or null
  GrxLane lane;                           // the overflow lane, entry mode only (include/grx_capi.h grx_sim_buffers)
};

// The second, optional output block (include/grx_capi.h grx_sim_dynamics): the site Jacobians, the mass matrix and the force / acceleration vectors of the LAST forward pass,
// what MjData holds next to the fields above.  Passed by value beside GrxSimBuffers; every pointer may be null.  A launch with a block of nulls runs the
// kernels without the block (csrc/grx_kernels.hip: DYN = false, d = nullptr).
#ifndef GRX_SIM_MAXJAC
#define GRX_SIM_MAXJAC 16   // include/grx_capi.h
#endif
struct GrxSimDynamics {
  float* qM;                                                       // [N,nv,nv] dense mj_fullM(data.qM)
  float *qfrc_smooth, *qacc_smooth, *qfrc_constraint, *qacc;       // [N,nv] persistent in GrxCtx
  float *qfrc_bias, *qfrc_passive, *qfrc_actuator;                 // [N,nv] P1 overlay: copied out between the velocity and the solve stage of the last pass
  float *site_jacp, *site_jacr;                                    // [N,njac,3,nv] mj_jacSite of the selected sites
  int njac, jac_site[GRX_SIM_MAXJAC];                              // the selection rides in the block: no device list, no dependent load
};

// The third, optional output block (include/grx_capi.h grx_sim_contacts): MjData's contact list of the LAST forward pass and mj_contactForce of every entry.  Passed by value
// beside the other two; every pointer may be null.  ccap slots per world, in the ENGINE's list order (sorted by candidate pair, not MuJoCo's order): a world writes its first
// min(ncon, table maxcon, ccap) slots and fills the rest (geom -1, dim 0, efc_address -1, floats 0.0f), so every element of a requested buffer is owed by the launch.
struct GrxSimContacts {
  int *geom, *dim, *efc_address;          // [N,ccap,2] [N,ccap] [N,ccap]: pair_geom1 / pair_geom2 of the contact's pair, its condim, its first constraint row (-1: none)
  float *dist, *pos, *frame, *force;      // [N,ccap] [N,ccap,3] [N,ccap,9] [N,ccap,6]: frame = normal and the two tangents of grx_make_frame, force in that frame
  int ccap;
};

// The fourth optional block (include/grx_capi.h grx_sim_applied), the stepper's only INPUT that is not an actuator: MjData's qfrc_applied and xfrc_applied, held over the
// substeps of a launch as ctrl is and never written, and xipos, the point xfrc_applied acts at, as an output of the same pass as xpos.  Every pointer may be null.  A launch
// with a pointer set runs the kernels of the units compiled with GRX_APPLIED_FORCES, whose velocity stage ends in grx_applied_forces (csrc/grx_eng_velocity.h).
struct GrxSimApplied {
  const float *qfrc_applied, *xfrc_applied;   // [N,nv] [N,nbody,6]: (force, torque) per compiled body in world coordinates, row 0 ignored
  float* xipos;                               // [N,nbody,3]
};

template <class S>
struct GrxSim {
  typedef GrxEngine<S> E;
  // data.xipos of the pass xpos is from: xpos + xmat body_ipos, the expression grx_inertia_cdof evaluates (both factors are persistent in GrxCtx); element e on lane e mod 64
  GRX_MEM void grx_sim_xipos_out(const GrxModel* m, const GrxCtx* c, float* xipos, size_t w, int lane_) {
    if (!xipos) return;
    GRX_FRESH_MODEL(m, c);
    const int nb = GRX_NBC;
    FOR_LANES {
      for (int e = lane; e < 3 * nb; e += 64) {
        const int b = e / 3, k = e - 3 * b;
        const float* R = c->xmat + 9 * b + 3 * k;
        xipos[w * 3 * nb + e] = c->xpos[e] + R[0] * m->body_ipos[3 * b] + R[1] * m->body_ipos[3 * b + 1] + R[2] * m->body_ipos[3 * b + 2];
      }
    }
  }
  // The contact list leaves in two parts, because the solve stage reuses the P1 overlay the list lives in (grx_ctx_carve) and efc_force exists only after the solve.
  // Part 1, between grx_make_constraint and the solve of the last pass: geom, dim, efc_address, dist, pos and frame.  A world's rows of a member are contiguous; one lane
  // writes one contact (GRX_MAXCON = 64: one lane per contact).  Lane k keeps what part 2 needs of the contact in OUTPUT SLOT k in two registers across the solve: crow = the
  // first row or -1, ckey = pair << 4 | rows.  A contact whose rows do not all lie inside nefc has none: address -1, zero force.
  GRX_MEM void grx_sim_contacts_p1(const GrxModel* m, const GrxCtx* c, const GrxSimContacts* o, size_t w, int lane_, int& crow, int& ckey) {
    GRX_FRESH_MODEL(m, c);
    const int ncon = c->cnt[0] < c->maxcon ? c->cnt[0] : c->maxcon, nefc = c->cnt[1], cap = o->ccap, nw = ncon < cap ? ncon : cap;
    // The ORDER of the outputs is by candidate pair, a pair's contacts in the engine's order: the order grx_collision's own re-sort leaves where it runs (noslip models, the
    // large scenes).  Elsewhere its late queues (box-box, hull pairs, large plane-mesh pairs) append their contacts behind the analytic ones, and the constraint rows are built
    // in that order: the list stays as it is -- a launch that requests contacts computes what one that does not computes -- and the outputs are permuted.  Lane k is contact k:
    // it ranks its contact by counting and writes it to slot `rank`; lane r then takes over what part 2 needs of the contact in slot r.
    FOR_LANES {
      int rank = lane, r0 = -1, nr = 0, p = 0;
      if (lane < ncon) {
        p = c->con_pair[lane];
        rank = 0;
        for (int j = 0; j < ncon; j++) { const int pj = c->con_pair[j]; rank += (pj < p) || (pj == p && j < lane); }
        r0 = c->con_efc[lane]; nr = c->con_nr[lane];
        if (!(r0 >= 0 && nr > 0 && r0 + nr <= nefc)) { r0 = -1; nr = 0; }
      }
      const int own_key = (p << 4) | nr;
      int src = lane;   // the contact in slot `lane`: ranks are a permutation of 0 .. ncon - 1, the lanes past the list keep their own (empty) registers
      for (int j = 0; j < ncon; j++) { if (__shfl(rank, j) == lane) src = j; }   // wave-uniform trip count
      crow = __shfl(r0, src); ckey = __shfl(own_key, src);
      if (lane < ncon && rank < cap) {
        const size_t s = w * cap + rank;
        if (o->efc_address) o->efc_address[s] = r0;
        if (o->dim) o->dim[s] = m->reci_pair[GRX_RPI * p];
        if (o->geom) { o->geom[2 * s] = m->pair_geom1[p]; o->geom[2 * s + 1] = m->pair_geom2[p]; }
        if (o->dist) o->dist[s] = c->con_dist[lane];
        if (o->pos) { for (int t = 0; t < 3; t++) o->pos[3 * s + t] = c->con_pos[3 * lane + t]; }
        if (o->frame) {   // the frame the contact's rows were built in: the same routine on the same normal (grx_make_constraint)
          float fr[9] = {c->con_frame[3 * lane], c->con_frame[3 * lane + 1], c->con_frame[3 * lane + 2], 0, 0, 0, 0, 0, 0};
          E::grx_make_frame(fr);
#pragma unroll
          for (int q = 0; q < 9; q++) o->frame[9 * s + q] = fr[q];
        }
      }
      for (int e = nw + lane; e < cap; e += 64) {   // the slots past the list: the fill values
        const size_t s = w * cap + e;
        if (o->efc_address) o->efc_address[s] = -1;
        if (o->dim) o->dim[s] = 0;
        if (o->geom) { o->geom[2 * s] = -1; o->geom[2 * s + 1] = -1; }
        if (o->dist) o->dist[s] = 0.0f;
        if (o->pos) { for (int t = 0; t < 3; t++) o->pos[3 * s + t] = 0.0f; }
        if (o->frame) { for (int q = 0; q < 9; q++) o->frame[9 * s + q] = 0.0f; }
      }
    }
  }
  // Part 2, after the pass: mj_contactForce for the pyramidal cone from the contact's rows of efc_force (P2 overlay, untouched since the solve), in flat order as above.  Lane
  // e mod 64 fetches the rows and the pair of contact e / 6 from the lane that kept them (every lane of the wave takes part in the exchange: the trip count is wave-uniform).
  // mu is the pair's friction row of THIS world's model (GRX_FRESH_MODEL: the world's own descriptor in the parameter units).
  GRX_MEM void grx_sim_contact_force(const GrxModel* m, GrxCtx* c, const GrxSimContacts* o, size_t w, int lane_, int crow, int ckey) {
    if (!o->force) return;
    GRX_FRESH_MODEL(m, c);
    const int ncon = c->cnt[0] < c->maxcon ? c->cnt[0] : c->maxcon, cap = o->ccap, nw = ncon < cap ? ncon : cap, total = 6 * cap, nefc = c->cnt[1];
    // grx_solve_integrate skips the evaluation at the converged acceleration where nothing reads the row forces afterwards (no touch sensor, no noslip pass): efc_force is
    // then one Newton step old.  Here something does read them: evaluate once more, from c->qacc and the persistent row tables (Ma, efc_jar and efc_quad, which the
    // evaluation also writes, are dead once the pass is over).  Where the engine did evaluate -- or noslip has re-solved the friction forces -- efc_force is left as it is.
    if (nefc > 0 && (S::kFixed ? S::NT : m->ntouch) == 0 && !(S::kNoslip && m->noslip_iterations > 0)) E::grx_newton_eval(m, c, c->qacc, nefc, 0, lane_);
    for (int base = 0; base < total; base += 64) {
      const int e = base + lane_, k = e / 6, j = e - 6 * k;
      const int r0 = __shfl(crow, k & 63), key = __shfl(ckey, k & 63);
      const int nr = key & 15, p = key >> 4, dim = (nr == 1) ? 1 : (nr >> 1) + 1;
      float v = 0.0f;
      if (e < total && k < nw && r0 >= 0) {
        if (j == 0) { for (int q = 0; q < nr; q++) v += c->efc_force[r0 + q]; }
        else if (j < dim) v = m->recf_pair[GRX_RPF * p + 3 + (j - 1)] * (c->efc_force[r0 + 2 * (j - 1)] - c->efc_force[r0 + 2 * (j - 1) + 1]);
      }
      if (e < total) o->force[w * total + e] = v;
    }
  }
  // grx_forward_euler's stage sequence with one addition: qfrc_bias / qfrc_passive / qfrc_actuator live in the P1 overlay, which the solve stage reuses (grx_ctx_carve), so
  // they leave for HBM between the velocity and the solve stage.  Only the LAST pass of a launch that asks for one of the three comes here; every other pass is
  // grx_forward_euler itself.  A world that claims a re-run on the large tables after this pass has written its three rows already: the re-run overwrites them.
  // CON: the instance of the launches that request a contact output (o, crow, ckey: grx_sim_contacts_p1); they come here in their last pass whatever d holds.
  template <bool CON>
  GRX_MEM void grx_sim_forward_p1(const GrxModel* m, GrxCtx* c, int do_euler, const GrxSimDynamics* d, const GrxSimContacts* o, int& crow, int& ckey, size_t w, int lane_) {
    GRX_TICK(c, GRX_P_OTHER);
    E::grx_kinematics(m, c, lane_);
    GRX_TICK(c, GRX_P_KIN);
    E::grx_inertia_cdof(m, c, lane_);
    GRX_TICK(c, GRX_P_INERTIA);
    E::grx_collision(m, c, lane_);
    if (S::kHandoff && (c->cnt[2] & GRX_ST_HULL)) return;
    GRX_TICK(c, GRX_P_COLLIDE);
    E::grx_make_constraint(m, c, lane_);
    if (grx_handoff_due(c)) return;
    GRX_TICK(c, GRX_P_CONSTR);
    if constexpr (CON) grx_sim_contacts_p1(m, c, o, w, lane_, crow, ckey);
    E::grx_velocity(m, c, lane_);
    {
      GRX_FRESH_MODEL(m, c);
      const int nv = GRX_NVC;
      FOR_LANES {
        if (lane < nv) {
          if (d->qfrc_bias) d->qfrc_bias[w * nv + lane] = c->qfrc_bias[lane];
          if (d->qfrc_passive) d->qfrc_passive[w * nv + lane] = c->qfrc_passive[lane];
          if (d->qfrc_actuator) d->qfrc_actuator[w * nv + lane] = c->qfrc_actuator[lane];
        }
      }
    }
#if defined(GRX_SIM_SENSORS)
    // the sensor block's two phases stand around the solve of the pass the readings belong to (csrc/grx_sim_sensors.h)
    if (c->sns_pass) GrxSns<S>::grx_sim_sensors_p1(m, c, c->sns, c->sns_row, lane_);
#endif
    E::grx_solve_integrate(m, c, do_euler, lane_);
#if defined(GRX_SIM_SENSORS)
    if (c->sns_pass) GrxSns<S>::grx_sim_sensors_p2(m, c, c->sns, c->sns_row, lane_);
#endif
  }
  // nstep x mj_step with ctrl held (GrxPoint::grx_point_sim_world with agent = 1 and no task: Euler models one pass per substep, RK4 models four), or one mj_forward.
  // A launch with an entry list (c->bail) stops at the first pass that exceeds a table: the world's re-run on the large tables is booked and nothing of this run is kept.
  // DYN = false: the instance of the launches that request nothing of GrxSimDynamics; d is null and not read.
  // CON = true (with DYN = true: those kernels carry both optional blocks): the instance of the launches that request a contact output.
  template <bool DYN, bool CON>
  GRX_MEM void grx_sim_world(const GrxModel* m, GrxCtx* c, int nstep, int forward_only, const GrxSimDynamics* d, const GrxSimContacts* o, int& crow, int& ckey, size_t w, int lane_) {
    const int p1 = CON || (DYN && ((d->qfrc_bias != nullptr) | (d->qfrc_passive != nullptr) | (d->qfrc_actuator != nullptr)));   // wave-uniform: kernel arguments
    if (forward_only) {
#if defined(GRX_SIM_SENSORS)
      c->sns_pass = c->sns != nullptr;
#endif
      if (p1) grx_sim_forward_p1<CON>(m, c, 0, d, o, crow, ckey, w, lane_);
      else E::grx_forward_euler(m, c, 0, lane_);
      if (c->bail) grx_lane_claim(c, lane_);
      return;
    }
    const int rk4 = (m->integrator == 1);
    const int total = rk4 ? 4 * nstep : nstep;
    for (int it = 0; it < total; it++) {
      const int stage = it & 3;
      if (!rk4 || stage == 0) E::grx_check_state(m, c, lane_);
#if defined(GRX_SIM_SENSORS)
      // sensordata belongs to the pass mj_step runs with sensors: the substep's own forward pass.  Euler: the last substep's only pass (the one the other outputs come from).
      // RK4: the FIRST stage's pass of the last substep -- mj_RungeKutta's further stages skip the sensors -- so that pass goes through grx_sim_forward_p1 as well; what it
      // writes of the other blocks there is written again by the fourth stage's pass.
      c->sns_pass = c->sns != nullptr && it == (rk4 ? total - 4 : total - 1);
      if ((p1 && it == total - 1) || c->sns_pass) grx_sim_forward_p1<CON>(m, c, !rk4, d, o, crow, ckey, w, lane_);
#else
      if (p1 && it == total - 1) grx_sim_forward_p1<CON>(m, c, !rk4, d, o, crow, ckey, w, lane_);
#endif
      else E::grx_forward_euler(m, c, !rk4, lane_);
      if (c->bail && grx_lane_claim(c, lane_)) break;
      if (rk4) E::grx_rk4_after_forward(m, c, stage, lane_);
    }
  }
  // The derived fields as MjData holds them now: those of the last forward pass (after a step: the position / velocity stage of the last substep, BEFORE its integration),
  // except the site velocities, which are J(site) of that pass times the CURRENT qvel -- mj_jacSite(model, data) @ data.qvel, what mujoco_utils.get_site_xvelp computes.
  // w: the world's row.  Strided per-lane copies straight from the context.
  GRX_MEM void grx_sim_outputs(const GrxModel* m, const GrxCtx* c, const GrxSimBuffers* b, size_t w, int lane_) {
    GRX_FRESH_MODEL(m, c);
    const int nb = GRX_NBC, ns = GRX_NSC;
    FOR_LANES {
      if (b->xpos) for (int i = lane; i < 3 * nb; i += 64) b->xpos[w * 3 * nb + i] = c->xpos[i];
      if (b->xquat) for (int i = lane; i < 4 * nb; i += 64) b->xquat[w * 4 * nb + i] = c->xquat[i];
      if (b->site_xpos) for (int i = lane; i < 3 * ns; i += 64) b->site_xpos[w * 3 * ns + i] = c->sxpos[i];
      if (b->site_xmat) for (int i = lane; i < 9 * ns; i += 64) b->site_xmat[w * 9 * ns + i] = c->sxmat[i];
      if (b->site_xvelp || b->site_xvelr)
        for (int s = lane; s < ns; s += 64) {
          float vp[3], vr[3];
          GrxFetch<S>::grx_point_velocity(m, c, m->site_bodyid[s], c->sxpos + 3 * s, vp, vr);
          if (b->site_xvelp) for (int k = 0; k < 3; k++) b->site_xvelp[w * 3 * ns + 3 * s + k] = vp[k];
          if (b->site_xvelr) for (int k = 0; k < 3; k++) b->site_xvelr[w * 3 * ns + 3 * s + k] = vr[k];
        }
    }
    if (b->sensordata && m->ntouch > 0) E::grx_touch_sensors(m, c, b->sensordata + w * m->ntouch, 1, lane_);   // raw mjSENS_TOUCH readings of the same pass as the contacts
    LANE0 {
      if (b->ncon) b->ncon[w] = c->cnt[0] < c->maxcon ? c->cnt[0] : c->maxcon;
      if (b->nefc) b->nefc[w] = c->cnt[1];
    }
  }
  // The second block, from the same pass.  Everything here reads persistent LDS; c->A and c->tmpv (P2 overlay, dead once the pass is over) serve as scratch.
  GRX_MEM void grx_sim_dynamics_out(const GrxModel* m, GrxCtx* c, const GrxSimDynamics* d, size_t w, int lane_) {
    GRX_FRESH_MODEL(m, c);
    const int nv = GRX_NVC;
    FOR_LANES {
      if (d->qM) for (int i = lane; i < nv * nv; i += 64) d->qM[w * nv * nv + i] = c->M[i];
      if (lane < nv) {
        if (d->qfrc_smooth) d->qfrc_smooth[w * nv + lane] = c->qfrc_smooth[lane];
        if (d->qfrc_constraint) d->qfrc_constraint[w * nv + lane] = c->qfrc_constraint[lane];
        if (d->qacc) d->qacc[w * nv + lane] = c->qacc[lane];
      }
    }
    if (d->qacc_smooth) {
      // The engine forms M^-1 qfrc_smooth only in a pass without constraint rows (grx_solve_integrate, phase 2); with rows Newton starts from the warm start and
      // c->qacc_smooth still holds qfrc_smooth.  MjData holds the unconstrained acceleration either way: solve here, in LDS, on a copy of M.
      if (c->cnt[1] > 0) {
        FOR_LANES {
          for (int i = lane; i < nv * nv; i += 64) c->A[i] = c->M[i];
          if (lane < nv) c->tmpv[lane] = c->qfrc_smooth[lane];
        }
        WAVE_SYNC();
        E::grx_sym_factor(c->A, nv, lane_);
        E::grx_sym_solve(c->A, nv, c->tmpv, lane_);
      }
      const float* qs = c->cnt[1] > 0 ? c->tmpv : c->qacc_smooth;
      FOR_LANES { if (lane < nv) d->qacc_smooth[w * nv + lane] = qs[lane]; }
    }
    // mj_jacSite of the selected sites, the arithmetic of GrxFetch<S>::grx_point_velocity column by column.  The njac blocks [3, nv] of a world are contiguous: element e of
    // the world's row goes to lane e mod 64, so every store instruction covers 64 consecutive words whatever njac and nv are.  A column off the body's dof chain (a site
    // on the world body: every column) is an exact zero; nothing is left to the caller's initialisation.
    if ((d->site_jacp || d->site_jacr) && d->njac > 0) {
      const int blk = 3 * nv, total = d->njac * blk;
      FOR_LANES {
        for (int e = lane; e < total; e += 64) {
          const int k = e / blk, rem = e - k * blk, r = rem / nv, col = rem - r * nv;
          int s = d->jac_site[0];
#pragma unroll
          for (int j = 1; j < GRX_SIM_MAXJAC; j++) s = (k == j) ? d->jac_site[j] : s;   // a select chain over kernel arguments: a lane-indexed read would move the block to scratch
          const int* CI = m->reci_chain + GRX_RCI * m->site_bodyid[s];   // dof chain mask lo / hi, root body
          const int on = (int)((col < 32 ? (unsigned)CI[0] >> col : (unsigned)CI[1] >> (col - 32)) & 1u);
          const float* cref = c->xpos + 3 * CI[2]; const float* point = c->sxpos + 3 * s; const float* cd = c->cdof + 6 * col;
          const float off[3] = {point[0] - cref[0], point[1] - cref[1], point[2] - cref[2]};
          float t[3]; cross3f(t, cd, off);
          const float tr = r == 0 ? t[0] : (r == 1 ? t[1] : t[2]);
          if (d->site_jacp) d->site_jacp[w * total + e] = on ? cd[3 + r] + tr : 0.0f;
          if (d->site_jacr) d->site_jacr[w * total + e] = on ? cd[r] : 0.0f;
        }
      }
    }
  }
};
