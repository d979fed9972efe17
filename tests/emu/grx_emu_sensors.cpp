// grx_emu_sensors.cpp -- TEST INFRASTRUCTURE: the lane emulator with the sensor block (gymnasium_robotics_amd/csrc/grx_sim_sensors.h), a library of its own beside
// libgrx_emu.so as grx_emu_rays.cpp is.  It includes the emulator's source, which stays as it is, and adds one entry point: the pass the readings belong to, stage by stage as
// GrxSim<S>::grx_sim_forward_p1 runs it on the device, with the two sensor phases around the solve.
//
// Built with -DGRX_EMU_SENSORS_ONLY it is a small library that holds only the two phases (emu_sns_p1 / emu_sns_p2): tests/test_cpu_sensors.py compiles MUTATED copies of the
// header that way and hands their phases to emu_sensors of the full library, so a mutation costs a two-second build and not a build of the engine.
#ifdef GRX_EMU_SENSORS_ONLY
#define GRX_EMU 1
#define GRX_HULL_HINTS 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <math.h>
#include <stdint.h>
typedef float grx_f32_t;
#ifndef GRX_SENSORS_HEADER
#define GRX_SENSORS_HEADER "../../gymnasium_robotics_amd/csrc/grx_sim_sensors.h"
#endif
#include GRX_SENSORS_HEADER
#else
#include "grx_emu.cpp"
#include "../../gymnasium_robotics_amd/csrc/grx_sim_sensors.h"
#endif

typedef void (*emu_sns_phase)(const GrxModel*, const GrxCtx*, const GrxSimSensors*, float*);

extern "C" {
void emu_sns_p1(const GrxModel* m, const GrxCtx* c, const GrxSimSensors* sn, float* row) { GrxSns<GrxShapeAny>::grx_sim_sensors_p1(m, c, sn, row, 0); }
void emu_sns_p2(const GrxModel* m, const GrxCtx* c, const GrxSimSensors* sn, float* row) { GrxSns<GrxShapeAny>::grx_sim_sensors_p2(m, c, sn, row, 0); }

#ifndef GRX_EMU_SENSORS_ONLY
// The readings of the loaded state (zero warm start): nstep = 0 after one forward pass; nstep > 0 after nstep physics steps as grx_sim_world runs them, from the pass mj_step
// runs with sensors -- an Euler model's last pass, the FIRST stage's pass of an RK4 model's last substep.  spec [nsensor, 4], cutoff [nsensor], out [ndata] (pre-filled by the
// caller: what the phases do not write stays).  p1 / p2: null, or the phases of another build of the header (above).  qacc [nv]: the pass's acceleration, or null.
void emu_sensors(void* h, const float* qpos, const float* qvel, const float* ctrl, const int* spec, const float* cutoff, int nsensor, int ndata, float* out, int nstep,
                 emu_sns_phase p1, emu_sns_phase p2, float* qacc) {
  Emu* e = (Emu*)h; typedef GrxEngine<GrxShapeAny> E;
  GrxCtx* c = &e->c; const GrxModel* m = &e->m;
  float mocap[8] = {0};
  for (int k = 0; k < m->nmocap && k < 1; k++) { memcpy(mocap, m->mocap_pos0, 12); memcpy(mocap + 3, m->mocap_quat0, 16); }
  std::vector<float> ws((size_t)m->nv + 1, 0.0f);
  load_state(e, qpos, qvel, ws.data(), mocap);
  for (int k = 0; k < m->nu; k++) c->ctrl[k] = ctrl ? ctrl[k] : 0.0f;
  GrxSimSensors sn; sn.spec = spec; sn.cutoff = cutoff; sn.nsensor = nsensor; sn.ndata = ndata; sn.data = out;
  if (!p1) p1 = emu_sns_p1;
  if (!p2) p2 = emu_sns_p2;
  const int rk4 = (m->integrator == 1), total = nstep <= 0 ? 1 : (rk4 ? 4 * nstep : nstep);
  for (int it = 0; it < total; it++) {
    const int stage = it & 3, do_euler = nstep > 0 && !rk4;
    if (nstep > 0 && (!rk4 || stage == 0)) E::grx_check_state(m, c, 0);
    if (nstep <= 0 || it == (rk4 ? total - 4 : total - 1)) {
      E::grx_kinematics(m, c, 0); E::grx_inertia_cdof(m, c, 0); E::grx_collision(m, c, 0); E::grx_make_constraint(m, c, 0); E::grx_velocity(m, c, 0);
      p1(m, c, &sn, out);
      E::grx_solve_integrate(m, c, do_euler, 0);
      p2(m, c, &sn, out);
      if (qacc) for (int k = 0; k < m->nv; k++) qacc[k] = (float)c->qacc[k];
    } else E::grx_forward_euler(m, c, do_euler, 0);
    if (nstep > 0 && rk4) E::grx_rk4_after_forward(m, c, stage, 0);
  }
}
#endif
}
