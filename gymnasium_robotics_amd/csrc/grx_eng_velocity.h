// grx_eng_velocity.h -- K4 - K7: body velocities, bias force (RNE), passive forces, actuation.
// A FRAGMENT of csrc/grx_engine.h: textually included INSIDE `template <class S> struct GrxEngine { ... }` (every function here is a static member), in the order the engine
// header lists; not a standalone header.  The split is purely textual (round 5): the token stream of the translation units is unchanged.
// ------------------------------------------------------------------------------------------
// velocity stage: cvel, cdof_dot, RNE bias (K2/K5), passive (K6), actuation (K7)
// ------------------------------------------------------------------------------------------
// generalised force of actuator i on the dof of its joint: gear * clamp(gain * clamp(ctrl) + bias), the arithmetic of grx_velocity's actuator loop; *next = the next actuator
// on the same dof, or -1.  Only the pass over shared dofs calls it.
GRX_MEM float grx_actuator_force(const GrxModel* m, const GrxCtx* c, int i, int* next) {
  const int* AI = m->reci_act + GRX_RAI * i; const float* AF = m->recf_act + GRX_RAF * i;
  const int qadr = AI[0], dadr = AI[1], ctrllimited = AI[2], gaintype = AI[3], biastype = AI[4], forcelimited = AI[5];
  const float gear = AF[0], cr0 = AF[1], cr1 = AF[2], g0 = AF[3], g1 = AF[4], g2 = AF[5], b0 = AF[6], b1 = AF[7], b2 = AF[8], fr0 = AF[9], fr1 = AF[10];
  float len = gear * c->qpos[qadr], vel = gear * c->qvel[dadr];
  float u = c->ctrl[i];
  if (ctrllimited) u = fminf(cr1, fmaxf(cr0, u));
  float gain = g0;
  if (gaintype == 1) gain += g1 * len + g2 * vel;
  float bias = 0;
  if (biastype == 1) bias = b0 + b1 * len + b2 * vel;
  float f = gain * u + bias;
  if (forcelimited) f = fminf(fr1, fmaxf(fr0, f));
  *next = AI[7];
  return gear * f;
}

#if defined(GRX_APPLIED_FORCES)
// Applied forces (mj_xfrcAccumulate and qfrc_applied), only in the units compiled with GRX_APPLIED_FORCES; called at the end of grx_velocity, so in every forward pass:
//   Q = qfrc_applied + sum over bodies b >= 1 of jacp_b' f_b + jacr_b' t_b,   qfrc_smooth += Q
// with (f_b, t_b) = xfrc_applied[b] in world coordinates and the Jacobians of xipos[b] = xpos[b] + xmat[b] body_ipos[b].  The bias force's scheme with another per-body vector:
// the spatial force of body b about its tree's reference point, (t_b + (xipos_b - cref) x f_b, f_b), takes cacc's place (dead once qfrc_bias is formed), the subtree sums
// take cfrc's, and dof d's lane dots its motion axis with the sum of its body.  One writer per element, no atomics.  The two rows are read from HBM in each pass (one lane per
// body and per dof, L2-resident after the first pass): no LDS is added.  grx_applied_load issues those loads at the TOP of the velocity stage, into seven registers per lane
// (a model has at most 64 bodies -- body_submask -- and 64 dofs: lane l holds body 1 + l and dof l), so their latency passes behind the stage's own work instead of standing
// between it and the solve.  Row 0 (the world body) is not read.  Either pointer may be null.
struct GrxAppliedRows { float x[6], q; };
GRX_MEM void grx_applied_load(const GrxModel* m, const GrxCtx* c, int lane_, GrxAppliedRows& r) {
  for (int k = 0; k < 6; k++) r.x[k] = 0.0f;
  r.q = 0.0f;
  const int b = 1 + lane_;
  if (c->xfrc_applied && b < GRX_NBC) { const float* x = c->xfrc_applied + 6 * b; for (int k = 0; k < 6; k++) r.x[k] = x[k]; }
  if (c->qfrc_applied && lane_ < GRX_NVC) r.q = c->qfrc_applied[lane_];
}
GRX_MEM void grx_applied_forces(const GrxModel* m, GrxCtx* c, int lane_, const GrxAppliedRows& ap) {
  if (!c->qfrc_applied && !c->xfrc_applied) return;   // wave-uniform: kernel arguments
  const int nv = GRX_NVC;
  if (c->xfrc_applied) {
    FOR_LANES {
      const int b = 1 + lane;
      if (b < GRX_NBC) {
        const float f[3] = {ap.x[0], ap.x[1], ap.x[2]}, t[3] = {ap.x[3], ap.x[4], ap.x[5]};
        const float* R = c->xmat + 9 * b; const float* cref = c->xpos + 3 * m->body_rootid[b];
        float ip[3] = {m->body_ipos[3 * b], m->body_ipos[3 * b + 1], m->body_ipos[3 * b + 2]}, r[3], rf[3];
        mulMatVec3f(r, R, ip);
        r[0] += c->xpos[3 * b] - cref[0]; r[1] += c->xpos[3 * b + 1] - cref[1]; r[2] += c->xpos[3 * b + 2] - cref[2];
        cross3f(rf, r, f);
        for (int k = 0; k < 3; k++) { c->cacc[6 * b + k] = t[k] + rf[k]; c->cacc[6 * b + 3 + k] = f[k]; }
      }
    }
    WAVE_SYNC();
    FOR_LANES {
      for (int it = lane; it < 6 * GRX_NBC; it += 64) {
        int b = it / 6, k = it - 6 * b;
        unsigned mlo = (unsigned)m->body_submask[2 * b], mhi = (S::kFixed && S::NB <= 32) ? 0u : (unsigned)m->body_submask[2 * b + 1];
        float s = 0;
#pragma unroll 16
        for (int e = 1; e < GRX_NBC; e++) { unsigned bit = e < 32 ? (mlo >> e) & 1u : (mhi >> (e - 32)) & 1u; s += bit ? c->cacc[6 * e + k] : 0.0f; }
        c->cfrc[it] = s;
      }
    }
    WAVE_SYNC();
  }
  FOR_LANES {
    if (lane < nv) {
      const int d = lane;
      float q = ap.q;
      if (c->xfrc_applied) {
        const int b = m->reci_dof[GRX_RDI * d + 6];
        float s = 0;
        for (int k = 0; k < 6; k++) s += c->cdof[6 * d + k] * c->cfrc[6 * b + k];
        q += s;
      }
      const float f = c->qfrc_smooth[d] + q;
      c->qfrc_smooth[d] = f; c->qacc_smooth[d] = f;
    }
  }
  WAVE_SYNC();
}
#endif

GRX_MEM void grx_velocity(const GrxModel* m, GrxCtx* c, int lane_) {
  GRX_OPAQUE_STAGE(lane_);   // record addresses and lane masks of this stage are recomputed here, not carried (spilled) across the substep loop
  GRX_FRESH_MODEL(m, c);
  const int nv = GRX_NVC;
#if defined(GRX_APPLIED_FORCES)
  GrxAppliedRows applied_rows;
  grx_applied_load(m, c, lane_, applied_rows);
#endif
  // One lane per dof (grx_model_create refuses more than 64): everything dof d's lane needs from the model in this stage comes from ONE record (GrxModel::reci_dof / recf_dof),
  // read in one volley -- the table walk it replaces (`j = dof_jntid[d]` ... `jnt_stiffness[j]` ... `jnt_qposadr[j]`, `dof_bodyid[dof_cvelstart[d]]` ... `body_dofadr[..]`) was
  // three dependent vector-L1 round trips (profiles/cpi_r06_fetch.txt).
  GRX_LANEVAR(damp); GRX_LANEVAR(stiff); GRX_LANEVAR(sref); GRX_LANEVAR_I(jqa); GRX_LANEVAR_I(jtyp); GRX_LANEVAR_I(jda); GRX_LANEVAR_I(ve0); GRX_LANEVAR_I(vbb); GRX_LANEVAR_I(vlast); GRX_LANEVAR_I(dbody);
  FOR_LANES {
    const int d = lane < nv ? lane : 0;
    const int* DI = m->reci_dof + GRX_RDI * d; const float* DF = m->recf_dof + GRX_RDF * d;
    LV(jqa) = DI[0]; LV(jtyp) = DI[1]; LV(jda) = DI[2]; LV(ve0) = DI[3]; LV(vbb) = DI[4]; LV(vlast) = DI[5]; LV(dbody) = DI[6];
    LV(damp) = DF[0]; LV(stiff) = DF[1]; LV(sref) = DF[2];
  }
  // The bias forces do not change when a whole tree is watched from a frame that moves with a constant linear velocity, and a free joint's three linear dofs are exactly
  // that for the tree below it: they are left out of the spatial velocities.  Carried along, they put terms of m |omega| |v| into cdof_dot and v x* I v that cancel in
  // qfrc_bias and cost it their fp32 rounding (a free root at 10 rad/s and 7 m/s, on the lane emulator: 3e-5 N on a bias of 11 N; 5e-6 N without them).  The generic engine
  // only: the kernels specialised for one family keep the arithmetic their free-running rollout records (tests/golden/tolerance_table.json) were measured with -- their
  // free bodies are slow -- and compile to what they compiled to before (nothing below exists in a fixed shape).
  unsigned long long flinmask = 0ull;
  if (!S::kFixed) {
    GRX_LANEVAR_I(flin);
    FOR_LANES { const int* DI = m->reci_dof + GRX_RDI * (lane < nv ? lane : 0); LV(flin) = (lane < nv && DI[1] == 0 && lane - DI[2] < 3) ? 1 : 0; }
    flinmask = GRX_BALLOT(flin);
  }
  // body spatial velocities = sum over the dof chain (parallel, no tree walk)
  FOR_LANES {
    for (int it = lane; it < 6 * GRX_NBC; it += 64) {
      int b = it / 6, k = it - 6 * b;
      unsigned mlo = (unsigned)m->dof_chainmask[2 * b], mhi = (unsigned)m->dof_chainmask[2 * b + 1];
      if (!S::kFixed) { mlo &= ~(unsigned)flinmask; mhi &= ~(unsigned)(flinmask >> 32); }
      float s = 0;
#pragma unroll 8
      for (int d = 0; d < nv; d++) { unsigned bit = d < 32 ? (mlo >> d) & 1u : (mhi >> (d - 32)) & 1u; s += bit ? c->cdof[6 * d + k] * c->qvel[d] : 0.0f; }
      c->cvel[it] = s;
    }
    // passive forces
    if (lane < nv) {
      const int d = lane;
      float f = -LV(damp) * c->qvel[d];
      if (LV(stiff) != 0.0f && LV(jtyp) >= 2) f -= LV(stiff) * (c->qpos[LV(jqa)] - LV(sref));
      c->qfrc_passive[d] = f;
      c->qfrc_actuator[d] = 0;
    }
  }
  WAVE_SYNC();
  FOR_LANES {
    // cdof_dot = crossMotion(velocity just before this dof, cdof).  That velocity is the spatial velocity of the body
    // owning dof_cvelstart[d], minus the dofs of that body that come after it (only multi-dof joints have any).
    if (lane < nv) {
      const int d = lane;
      float v[6] = {0, 0, 0, 0, 0, 0}, cd[6], r[6];
      const int e0 = LV(ve0);
      if (e0 >= 0) {
        const int bb = LV(vbb), last = LV(vlast);
        for (int k = 0; k < 6; k++) v[k] = c->cvel[6 * bb + k];
        for (int e = e0 + 1; e <= last; e++) { float qd = c->qvel[e]; for (int k = 0; k < 6; k++) v[k] -= c->cdof[6 * e + k] * qd; }
      }
      for (int k = 0; k < 6; k++) cd[k] = c->cdof[6 * d + k];
      if (LV(jtyp) == 0 && d - LV(jda) < 3) { for (int k = 0; k < 6; k++) r[k] = 0; }
      else crossMotionf(r, v, cd);
      for (int k = 0; k < 6; k++) c->cdof_dot[6 * d + k] = r[k];
    }
  }
  WAVE_SYNC();
  GRX_SUBTICK(c, 6);
  FOR_LANES {
    // accelerations with qacc = 0 and per-body inertial forces
    for (int b = 1 + lane; b < GRX_NBC; b += 64) {
      float a[6] = {0, 0, 0, -m->gravity[0], -m->gravity[1], -m->gravity[2]}, v[6], Ia[6], Iv[6], t[6];
      unsigned mlo = (unsigned)m->dof_chainmask[2 * b], mhi = (unsigned)m->dof_chainmask[2 * b + 1];
#pragma unroll 4
      for (int d = 0; d < nv; d++) {
        unsigned bit = d < 32 ? (mlo >> d) & 1u : (mhi >> (d - 32)) & 1u;
        float qd = bit ? c->qvel[d] : 0.0f;
        for (int k = 0; k < 6; k++) a[k] += c->cdof_dot[6 * d + k] * qd;
      }
      for (int k = 0; k < 6; k++) v[k] = c->cvel[6 * b + k];
      inertMulf(Ia, c->cinert + 10 * b, a); inertMulf(Iv, c->cinert + 10 * b, v);
      crossForcef(t, v, Iv);
      for (int k = 0; k < 6; k++) c->cacc[6 * b + k] = Ia[k] + t[k];
    }
    // actuators (one lane each; joint transmission)
    for (int i = lane; i < GRX_NUC; i += 64) {
      // one record per actuator (GrxModel::reci_act / recf_act), every field read up front: the flags used to guard the reads of the values they select, one round trip each
      const int* AI = m->reci_act + GRX_RAI * i; const float* AF = m->recf_act + GRX_RAF * i;
      const int qadr = AI[0], dadr = AI[1], ctrllimited = AI[2], gaintype = AI[3], biastype = AI[4], forcelimited = AI[5];
      const float gear = AF[0], cr0 = AF[1], cr1 = AF[2], g0 = AF[3], g1 = AF[4], g2 = AF[5], b0 = AF[6], b1 = AF[7], b2 = AF[8], fr0 = AF[9], fr1 = AF[10];
      float len = gear * c->qpos[qadr], vel = gear * c->qvel[dadr];
      float u = c->ctrl[i];
      if (ctrllimited) u = fminf(cr1, fmaxf(cr0, u));
      float gain = g0;
      if (gaintype == 1) gain += g1 * len + g2 * vel;
      float bias = 0;
      if (biastype == 1) bias = b0 + b1 * len + b2 * vel;
      float f = gain * u + bias;
      if (forcelimited) f = fminf(fr1, fmaxf(fr0, f));
      c->qfrc_actuator[dadr] = gear * f;  // the whole force of a dof with one actuator; a dof with several is written again below
    }
  }
  WAVE_SYNC();
  GRX_SUBTICK(c, 7);
  // Dofs with more than one actuator (a <position> plus a <velocity> on one joint is the usual PD pair): qfrc_actuator[d] is the SUM over the dof's actuators in actuator
  // order, the oracle's order.  The store above leaves one of the summands there, which one is not specified; here the lane of the dof's FIRST actuator walks the chain of
  // its actuators (record slots 6 and 7, grx_host_model.h), sums and writes once -- one writer per dof, no atomics.  The branch is wave-uniform, and the fixed shapes do not
  // carry it at all (GrxShape::kActShare): in their kernels the test costs a scalar load and a wait per substep, 0.4 % of a Fetch step when it was measured.
  if (S::kActShare && m->nactshare) {
    FOR_LANES {
      for (int i = lane; i < GRX_NUC; i += 64) {
        const int* AI = m->reci_act + GRX_RAI * i;
        if (AI[6]) {
          int next;
          float f = grx_actuator_force(m, c, i, &next);
          while (next >= 0) f += grx_actuator_force(m, c, next, &next);
          c->qfrc_actuator[AI[1]] = f;
        }
      }
    }
  }
  FOR_LANES {
    // subtree force sums
    for (int it = lane; it < 6 * GRX_NBC; it += 64) {
      int b = it / 6, k = it - 6 * b;
      unsigned mlo = (unsigned)m->body_submask[2 * b], mhi = (S::kFixed && S::NB <= 32) ? 0u : (unsigned)m->body_submask[2 * b + 1];
      float s = 0;
#pragma unroll 16
      for (int e = 1; e < GRX_NBC; e++) { unsigned bit = e < 32 ? (mlo >> e) & 1u : (mhi >> (e - 32)) & 1u; s += bit ? c->cacc[6 * e + k] : 0.0f; }
      c->cfrc[it] = s;
    }
  }
  WAVE_SYNC();
  GRX_SUBTICK(c, 8);
  FOR_LANES {
    if (lane < nv) {
      const int d = lane;
      float s = 0; int b = LV(dbody);
      for (int k = 0; k < 6; k++) s += c->cdof[6 * d + k] * c->cfrc[6 * b + k];
      c->qfrc_bias[d] = s;
      float f = c->qfrc_passive[d] - s + c->qfrc_actuator[d];
      c->qfrc_smooth[d] = f; c->qacc_smooth[d] = f;
    }
  }
  WAVE_SYNC();
#if defined(GRX_APPLIED_FORCES)
  grx_applied_forces(m, c, lane_, applied_rows);
#endif
}

