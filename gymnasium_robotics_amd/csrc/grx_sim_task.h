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

template <class S>
struct GrxSim {
  typedef GrxEngine<S> E;
  // grx_forward_euler's stage sequence with one addition: qfrc_bias / qfrc_passive / qfrc_actuator live in the P1 overlay, which the solve stage reuses (grx_ctx_carve), so
  // they leave for HBM between the velocity and the solve stage.  Only the LAST pass of a launch that asks for one of the three comes here; every other pass is
  // grx_forward_euler itself.  A world that claims a re-run on the large tables after this pass has written its three rows already: the re-run overwrites them.
  GRX_MEM void grx_sim_forward_p1(const GrxModel* m, GrxCtx* c, int do_euler, const GrxSimDynamics* d, size_t w, int lane_) {
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
    E::grx_solve_integrate(m, c, do_euler, lane_);
  }
  // nstep x mj_step with ctrl held (GrxPoint::grx_point_sim_world with agent = 1 and no task: Euler models one pass per substep, RK4 models four), or one mj_forward.
  // A launch with an entry list (c->bail) stops at the first pass that exceeds a table: the world's re-run on the large tables is booked and nothing of this run is kept.
  // DYN = false: the instance of the launches that request nothing of GrxSimDynamics; d is null and not read.
  template <bool DYN>
  GRX_MEM void grx_sim_world(const GrxModel* m, GrxCtx* c, int nstep, int forward_only, const GrxSimDynamics* d, size_t w, int lane_) {
    const int p1 = DYN && ((d->qfrc_bias != nullptr) | (d->qfrc_passive != nullptr) | (d->qfrc_actuator != nullptr));   // wave-uniform: kernel arguments
    if (forward_only) {
      if (p1) grx_sim_forward_p1(m, c, 0, d, w, lane_);
      else E::grx_forward_euler(m, c, 0, lane_);
      if (c->bail) grx_lane_claim(c, lane_);
      return;
    }
    const int rk4 = (m->integrator == 1);
    const int total = rk4 ? 4 * nstep : nstep;
    for (int it = 0; it < total; it++) {
      const int stage = it & 3;
      if (!rk4 || stage == 0) E::grx_check_state(m, c, lane_);
      if (p1 && it == total - 1) grx_sim_forward_p1(m, c, !rk4, d, w, lane_);
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
