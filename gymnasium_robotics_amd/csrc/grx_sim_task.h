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

template <class S>
struct GrxSim {
  typedef GrxEngine<S> E;
  // nstep x mj_step with ctrl held (GrxPoint::grx_point_sim_world with agent = 1 and no task: Euler models one pass per substep, RK4 models four), or one mj_forward.
  // A launch with an entry list (c->bail) stops at the first pass that exceeds a table: the world's re-run on the large tables is booked and nothing of this run is kept.
  GRX_MEM void grx_sim_world(const GrxModel* m, GrxCtx* c, int nstep, int forward_only, int lane_) {
    if (forward_only) {
      E::grx_forward_euler(m, c, 0, lane_);
      if (c->bail) grx_lane_claim(c, lane_);
      return;
    }
    const int rk4 = (m->integrator == 1);
    const int total = rk4 ? 4 * nstep : nstep;
    for (int it = 0; it < total; it++) {
      const int stage = it & 3;
      if (!rk4 || stage == 0) E::grx_check_state(m, c, lane_);
      E::grx_forward_euler(m, c, !rk4, lane_);
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
};
