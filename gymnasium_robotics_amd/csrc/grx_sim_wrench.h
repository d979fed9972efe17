// grx_sim_wrench.h -- the sixth optional block of the task-free stepper (include/grx_capi.h grx_sim_wrenches): what mj_rnePostConstraint forms per body -- subtree_com,
// cfrc_ext, cacc, cfrc_int -- and the force / torque sensors that read cfrc_int.  Only in the units compiled with GRX_SIM_WRENCHES (rows simwrn / simwrnprm of GRX_SIM_UNITS).
//
// FRAME.  Rows are MuJoCo's: six numbers per compiled body, rotation part first (torque, then force; angular, then linear), world orientation, about
// subtree_com[body_rootid[b]].  The engine's own spatial vectors are about cref = xpos[body_rootid[b]] (csrc/grx_eng_kinematics.h); a force vector moves to the point
// cref + r as tau' = tau - r x f, a motion vector as a_lin' = a_lin + alpha x r, once per body.  The world body's row is about subtree_com[0], the centre of mass of
// everything; what it sums comes from other trees and moves by the difference of the two reference points as it is added.
//
// ONE PASS, TWO PHASES around its solve, for the reason the sensor block has (csrc/grx_sim_sensors.h): cvel, cinert and cdof_dot live in the P1 overlay the solve reuses,
// qacc and efc_force exist after it.  One lane per body (a model has at most 64) and one lane per contact (GRX_MAXCON = 64).
//   phase 1, after grx_velocity: body b's lane forms the halves without qacc,
//              a0_b = (0, -g) + sum_chain cdof_dot[d] qvel[d]          f0_b = cinert_b a0_b + cvel_b x* (cinert_b cvel_b)
//            from the stage's own arrays (c->cacc / c->cfrc hold the applied wrenches by then: they are not read).  Contact k's lane takes the contact's position, normal,
//            first row and pair | row count, as grx_sim_contacts_p1 does.
//   phase 2, after the solve: ja_b = sum_chain cdof[d] qacc[d] (cdof is persistent), cacc_b = a0_b + ja_b, f_b = f0_b + cinert_b ja_b.
// WHAT CROSSES THE SOLVE crosses it in REGISTERS (GrxWrnKeep: 20 words per lane; the compiler may park them in scratch): the output rows are optional, a launch that only
// serves a force sensor has none, and no LDS is added -- grx_ctx_words and grx_ctx_carve are untouched.  cinert is NOT carried: phase 2 rebuilds it from the persistent
// xpos / xmat and the model's inertial tables with the expression of grx_inertia_cdof (same operands, same order: the same bits), 10 words per lane less across the solve.
// WHAT CROSSES LANES in phase 2 -- subtree sums over body_submask, contact k's wrench to the lanes of its two bodies, a sensor's body row -- crosses through the wave's
// cross-lane network (__shfl), every exchange in wave-uniform control flow, with one writer per body and no atomics.  Nothing is staged in LDS: what is provably dead of the
// P2 overlay after the solve (A, the Newton vectors, efc_jar / efc_jv) is nv^2 + 5 nv + 2 maxefc words, which a caller's own capacity= can make smaller than 6 (nbody + ncon),
// and efc_force above it is still read by grx_sim_contact_force.  For the same reason phase 2 is device code only (as grx_sim_contacts_p1 is); the lane emulator does not
// compile this header.
//
// CONTACTS.  The force of contact k in its frame is mj_contactForce exactly as grx_sim_contact_force forms it (pyramidal rows, the pair's friction of THIS world's model,
// after one more grx_newton_eval where nothing else forced the evaluation at the converged acceleration: the evaluation is a pure function of qacc and the persistent row
// tables, so the contact block's own evaluation after it reproduces the same bits).  With (n, t1, t2) = grx_make_frame(normal): F = n f0 + t1 f1 + t2 f2 acts on the body of
// the pair's second geom at contact_pos, with the free torque T = n f3 + t1 f4 + t2 f5 (torsional, rolling); the body of the first geom receives the opposite.  The lever
// arm is taken from the receiving body's own subtree_com[root] directly, not from cref and shifted.
//
// THE FREE JOINT.  The generic engine leaves a free joint's three linear dofs out of cvel and zeroes their cdof_dot (grx_eng_velocity.h, flinmask): it watches the tree from
// a frame that moves with v0 = that linear velocity, held constant.  Forces do not change under that boost: f0, cfrc_int and cfrc_ext need nothing.  A spatial acceleration
// does.  Its linear part is the classical acceleration of the body point at the reference point minus omega x (that point's velocity); the classical acceleration is the
// same in both frames, the point's velocity is larger by v0 in MuJoCo's, so
//   cacc_lin (MuJoCo) = cacc_lin (reduced frame) - omega_b x v0,     v0 = sum over the free linear dofs d in b's chain of cdof_lin[d] qvel[d].
// omega_b and v0 are phase 1 values (the Euler stage has replaced qvel by phase 2), so the term is folded into a0's linear part there.  The angular part needs nothing.
#pragma once
#include "grx_engine.h"
#include "grx_sim_sensors.h"

// The block as the kernels see it: the four pointers of grx_sim_wrenches (each may be null) and, filled in by the host, the number of force / torque rows of the sensor table.
struct GrxSimWrenches {
  float *cfrc_ext, *cfrc_int, *cacc, *subtree_com;   // [N,nbody,6] x 3, [N,nbody,3]
  int nft;
};
// what a lane keeps across the solve: of its body (a0 with the free-joint term folded in, f0), of its contact (position, normal, first row or -1, pair << 4 | rows)
struct GrxWrnKeep { float a0[6], f0[6], cp[3], cn[3]; int crow, ckey; };
enum { GRX_WRN_ROWS = 1, GRX_WRN_SENSORS = 2 };   // GrxCtx::wrn_pass: the pass that is running owes the body rows / the force and torque readings

#if defined(GRX_SIM_WRENCHES)   // the routines read the GrxCtx members of the units compiled with GRX_APPLIED_FORCES, GRX_SIM_SENSORS and GRX_SIM_WRENCHES
template <class S>
struct GrxWrn {
  typedef GrxEngine<S> E;
  GRX_MEM int grx_wrn_bit(unsigned lo, unsigned hi, int e) { return (int)((e < 32 ? lo >> e : hi >> (e - 32)) & 1u); }

  // Phase 1 (header).  Needs the pass's own qvel, cvel, cinert, cdof_dot and contact list: call it between grx_velocity and the solve.
  GRX_MEM void grx_sim_wrench_p1(const GrxModel* m, const GrxCtx* c, GrxWrnKeep& k, int lane_) {
    GRX_FRESH_MODEL(m, c);
    const int nv = GRX_NVC, nb = GRX_NBC;
    const int ncon = c->cnt[0] < c->maxcon ? c->cnt[0] : c->maxcon, nefc = c->cnt[1];
    const int b = lane_;
    for (int e = 0; e < 3; e++) { k.a0[e] = 0.0f; k.a0[3 + e] = -m->gravity[e]; k.f0[e] = k.f0[3 + e] = 0.0f; k.cp[e] = k.cn[e] = 0.0f; }   // row 0: cacc = (0, -g), no inertia
    k.crow = -1; k.ckey = 0;
    if (b >= 1 && b < nb) {
      const unsigned mlo = (unsigned)m->dof_chainmask[2 * b], mhi = (unsigned)m->dof_chainmask[2 * b + 1];
      float a[6] = {0, 0, 0, -m->gravity[0], -m->gravity[1], -m->gravity[2]}, v0[3] = {0, 0, 0}, v[6], Ia[6], Iv[6], t[6], wv[3];
#pragma unroll 4
      for (int d = 0; d < nv; d++) {
        const float qd = grx_wrn_bit(mlo, mhi, d) ? c->qvel[d] : 0.0f;
        for (int e = 0; e < 6; e++) a[e] += c->cdof_dot[6 * d + e] * qd;
        const int* DI = m->reci_dof + GRX_RDI * d;   // wave-uniform: joint type and first dof of the joint
        if (!S::kFixed && DI[1] == 0 && d - DI[2] < 3) { for (int e = 0; e < 3; e++) v0[e] += c->cdof[6 * d + 3 + e] * qd; }
      }
      for (int e = 0; e < 6; e++) v[e] = c->cvel[6 * b + e];
      inertMulf(Ia, c->cinert + 10 * b, a); inertMulf(Iv, c->cinert + 10 * b, v);
      crossForcef(t, v, Iv);
      cross3f(wv, v, v0);   // omega_b x v0 (header, THE FREE JOINT)
      for (int e = 0; e < 6; e++) k.f0[e] = Ia[e] + t[e];
      for (int e = 0; e < 3; e++) { k.a0[e] = a[e]; k.a0[3 + e] = a[3 + e] - wv[e]; }
    }
    if (lane_ < ncon) {
      int r0 = c->con_efc[lane_], nr = c->con_nr[lane_];
      if (!(r0 >= 0 && nr > 0 && r0 + nr <= nefc)) { r0 = -1; nr = 0; }   // the rule of grx_sim_contacts_p1: rows that do not all lie inside nefc are none
      k.crow = r0; k.ckey = (c->con_pair[lane_] << 4) | nr;
      for (int e = 0; e < 3; e++) { k.cp[e] = c->con_pos[3 * lane_ + e]; k.cn[e] = c->con_frame[3 * lane_ + e]; }
    }
  }

  // Phase 2 (header): after the solve of the same pass.  Needs qacc, efc_force and the persistent cdof, xpos, xmat, sxpos, sxmat; never qvel.  w: the world's row.
  // pass: GRX_WRN_* -- which of the rows of o and of the force / torque readings of c->sns this pass owes.
  GRX_MEM void grx_sim_wrench_p2(const GrxModel* m, GrxCtx* c, const GrxSimWrenches* o, const GrxWrnKeep& k, int pass, size_t w, int lane_) {
    GRX_FRESH_MODEL(m, c);
    const int nv = GRX_NVC, nb = GRX_NBC;
    const int ncon = c->cnt[0] < c->maxcon ? c->cnt[0] : c->maxcon, nefc = c->cnt[1];
    if (nefc > 0 && (S::kFixed ? S::NT : m->ntouch) == 0 && !(S::kNoslip && m->noslip_iterations > 0)) E::grx_newton_eval(m, c, c->qacc, nefc, 0, lane_);
    const int live = lane_ < nb, b = live ? lane_ : 0, root = m->body_rootid[b];
    const unsigned slo = (unsigned)m->body_submask[2 * b], shi = (unsigned)m->body_submask[2 * b + 1];
    const float* R = c->xmat + 9 * b; const float* xp = c->xpos + 3 * b; const float* cref = c->xpos + 3 * root;
    const float ip[3] = {m->body_ipos[3 * b], m->body_ipos[3 * b + 1], m->body_ipos[3 * b + 2]};
    const float mass = live ? m->body_mass[b] : 0.0f;
    float rl[3], xi[3];
    mulMatVec3f(rl, R, ip);
    for (int e = 0; e < 3; e++) xi[e] = xp[e] + rl[e];   // xipos_b, the expression of grx_sim_xipos_out
    // subtree_com_b = sum m_e xipos_e / sum m_e over the subtree, summed relative to xipos_b; a massless subtree has it at xipos_b (MuJoCo's rule)
    float sm = 0.0f, sx[3] = {0, 0, 0}, com[3], cr[3];
    for (int e = 0; e < nb; e++) {
      const float me = __shfl(mass, e), x0 = __shfl(xi[0], e), x1 = __shfl(xi[1], e), x2 = __shfl(xi[2], e);
      if (b == 0 || grx_wrn_bit(slo, shi, e)) { sm += me; sx[0] += me * (x0 - xi[0]); sx[1] += me * (x1 - xi[1]); sx[2] += me * (x2 - xi[2]); }
    }
    for (int e = 0; e < 3; e++) com[e] = sm >= GRX_MINVAL ? xi[e] + sx[e] / sm : xi[e];
    for (int e = 0; e < 3; e++) cr[e] = __shfl(com[e], root);   // the point b's rows are about
    // the body's own inertial wrench and acceleration, about cref, then about cr
    float ja[6] = {0, 0, 0, 0, 0, 0}, f[6], acc[6];
    {
      const unsigned mlo = (unsigned)m->dof_chainmask[2 * b], mhi = (unsigned)m->dof_chainmask[2 * b + 1];
#pragma unroll 4
      for (int d = 0; d < nv; d++) {
        const float qa = (b >= 1 && grx_wrn_bit(mlo, mhi, d)) ? c->qacc[d] : 0.0f;
        for (int e = 0; e < 6; e++) ja[e] += c->cdof[6 * d + e] * qa;
      }
    }
    for (int e = 0; e < 6; e++) { f[e] = k.f0[e]; acc[e] = k.a0[e] + ja[e]; }
    if (b >= 1) {   // cinert_b as grx_inertia_cdof forms it
      const float* in = m->body_inertia + 6 * b;
      float r[3] = {rl[0] + (xp[0] - cref[0]), rl[1] + (xp[1] - cref[1]), rl[2] + (xp[2] - cref[2])};
      float Ib[9] = {in[0], in[3], in[4], in[3], in[1], in[5], in[4], in[5], in[2]}, t[9], Rt[9], Iw[9], I[10], Ia[6];
      for (int a = 0; a < 3; a++) for (int e = 0; e < 3; e++) Rt[3 * a + e] = R[3 * e + a];
      mulMat3f(t, R, Ib); mulMat3f(Iw, t, Rt);
      const float rr = dot3f(r, r);
      I[0] = Iw[0] + mass * (rr - r[0] * r[0]); I[1] = Iw[4] + mass * (rr - r[1] * r[1]); I[2] = Iw[8] + mass * (rr - r[2] * r[2]);
      I[3] = Iw[1] - mass * r[0] * r[1]; I[4] = Iw[2] - mass * r[0] * r[2]; I[5] = Iw[5] - mass * r[1] * r[2];
      I[6] = mass * r[0]; I[7] = mass * r[1]; I[8] = mass * r[2]; I[9] = mass;
      inertMulf(Ia, I, ja);
      for (int e = 0; e < 6; e++) f[e] += Ia[e];
    }
    {
      const float r[3] = {cr[0] - cref[0], cr[1] - cref[1], cr[2] - cref[2]};
      float rf[3], ar[3];
      cross3f(rf, r, f + 3); cross3f(ar, acc, r);
      for (int e = 0; e < 3; e++) { f[e] -= rf[e]; acc[3 + e] += ar[e]; }
    }
    // cfrc_ext_b about cr: the applied wrench at xipos_b, then every contact of the pass on its two bodies
    float ext[6] = {0, 0, 0, 0, 0, 0};
    if (c->xfrc_applied && live && b >= 1) {
      const float* x = c->xfrc_applied + 6 * b;   // (force, torque) in world coordinates
      const float fa[3] = {x[0], x[1], x[2]}, lv[3] = {xi[0] - cr[0], xi[1] - cr[1], xi[2] - cr[2]};
      float lf[3]; cross3f(lf, lv, fa);
      for (int e = 0; e < 3; e++) { ext[e] = x[3 + e] + lf[e]; ext[3 + e] = fa[e]; }
    }
    {
      const int r0 = k.crow, nr = k.ckey & 15, p = k.ckey >> 4, dim = (nr == 1) ? 1 : (nr >> 1) + 1;
      float cf[6] = {0, 0, 0, 0, 0, 0}, fr[9] = {k.cn[0], k.cn[1], k.cn[2], 0, 0, 0, 0, 0, 0}, F[3], T[3];
      int cb1 = -1, cb2 = -1;
      if (lane_ < ncon && r0 >= 0) {
        for (int q = 0; q < nr; q++) cf[0] += c->efc_force[r0 + q];
        for (int j = 1; j < 6; j++) { if (j < dim) cf[j] = m->recf_pair[GRX_RPF * p + 3 + (j - 1)] * (c->efc_force[r0 + 2 * (j - 1)] - c->efc_force[r0 + 2 * (j - 1) + 1]); }
        cb1 = m->reci_pair[GRX_RPI * p + 3]; cb2 = m->reci_pair[GRX_RPI * p + 4];
      }
      E::grx_make_frame(fr);   // the frame the contact's rows were built in (a lane without a contact: a zero normal, finite tangents, zero force)
      for (int e = 0; e < 3; e++) { F[e] = fr[e] * cf[0] + fr[3 + e] * cf[1] + fr[6 + e] * cf[2]; T[e] = fr[e] * cf[3] + fr[3 + e] * cf[4] + fr[6 + e] * cf[5]; }
      for (int j = 0; j < ncon; j++) {   // wave-uniform trip count; body b's lane is the only writer of ext
        const int b1 = __shfl(cb1, j), b2 = __shfl(cb2, j);
        const float Fj[3] = {__shfl(F[0], j), __shfl(F[1], j), __shfl(F[2], j)}, Tj[3] = {__shfl(T[0], j), __shfl(T[1], j), __shfl(T[2], j)};
        const float lv[3] = {__shfl(k.cp[0], j) - cr[0], __shfl(k.cp[1], j) - cr[1], __shfl(k.cp[2], j) - cr[2]};
        const float sgn = (float)((lane_ == b2) - (lane_ == b1));
        float lf[3]; cross3f(lf, lv, Fj);
        if (sgn != 0.0f) { for (int e = 0; e < 3; e++) { ext[e] += sgn * (Tj[e] + lf[e]); ext[3 + e] += sgn * Fj[e]; } }
      }
    }
    // cfrc_int_b = sum over the subtree of (f_e - ext_e); an addend about another point (row 0 only) moves to cr as it is added
    float g[6], fi[6] = {0, 0, 0, 0, 0, 0};
    for (int e = 0; e < 6; e++) g[e] = f[e] - ext[e];
    for (int e = 0; e < nb; e++) {
      const float ge[6] = {__shfl(g[0], e), __shfl(g[1], e), __shfl(g[2], e), __shfl(g[3], e), __shfl(g[4], e), __shfl(g[5], e)};
      const float dv[3] = {__shfl(cr[0], e) - cr[0], __shfl(cr[1], e) - cr[1], __shfl(cr[2], e) - cr[2]};
      float df[3]; cross3f(df, dv, ge + 3);
      if (b == 0 || grx_wrn_bit(slo, shi, e)) { for (int q = 0; q < 3; q++) { fi[q] += ge[q] + df[q]; fi[3 + q] += ge[3 + q]; } }
    }
    if ((pass & GRX_WRN_ROWS) && live) {
      const size_t row = w * nb + b;
      if (o->subtree_com) for (int e = 0; e < 3; e++) o->subtree_com[3 * row + e] = com[e];
      if (o->cfrc_ext) for (int e = 0; e < 6; e++) o->cfrc_ext[6 * row + e] = ext[e];
      if (o->cacc) for (int e = 0; e < 6; e++) o->cacc[6 * row + e] = acc[e];
      if (o->cfrc_int) for (int e = 0; e < 6; e++) o->cfrc_int[6 * row + e] = fi[e];
    }
    // force / torque sensors: sensor s on lane s mod 64 fetches cfrc_int and the reference point of its site's body from that body's lane
    if ((pass & GRX_WRN_SENSORS) && c->sns) {
      const GrxSimSensors* sn = c->sns;
      for (int base = 0; base < sn->nsensor; base += 64) {   // wave-uniform
        const int s = base + lane_ < sn->nsensor ? base + lane_ : 0;
        const int* sp = sn->spec + 4 * s;
        const int type = sp[0], id = sp[2], adr = sp[3], on = base + lane_ < sn->nsensor && type >= GRX_SNS_FORCE;
        const int sb = on ? m->site_bodyid[id] : 0;
        const float tq[3] = {__shfl(fi[0], sb), __shfl(fi[1], sb), __shfl(fi[2], sb)}, fo[3] = {__shfl(fi[3], sb), __shfl(fi[4], sb), __shfl(fi[5], sb)};
        const float cs[3] = {__shfl(cr[0], sb), __shfl(cr[1], sb), __shfl(cr[2], sb)};
        if (on) {
          const float* ps = c->sxpos + 3 * id; const float* Rs = c->sxmat + 9 * id;
          const float lv[3] = {ps[0] - cs[0], ps[1] - cs[1], ps[2] - cs[2]};
          float lf[3], v[3]; cross3f(lf, lv, fo);
          for (int e = 0; e < 3; e++) v[e] = type == GRX_SNS_FORCE ? fo[e] : tq[e] - lf[e];
          const float cut = sn->cutoff[s];
          for (int e = 0; e < 3; e++) c->sns_row[adr + e] = GrxSns<S>::grx_sensor_clamp(Rs[e] * v[0] + Rs[3 + e] * v[1] + Rs[6 + e] * v[2], cut);   // R' v
        }
      }
    }
  }
};
#endif
