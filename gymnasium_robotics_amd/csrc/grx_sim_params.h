// grx_sim_params.h -- per-world model parameters of the task-free stepper (include/grx_capi.h grx_sim_params_*): which tables can be per world, the record-fill functions
// shared by the host and the commit kernels, the commit's validation rules and the two commit kernels' bodies.
//
// A parameter object holds for every world (a) a row of each named table that the caller writes (the STAGE rows), (b) the committed copy of those rows plus a private copy of
// the float records that are gathered from them (the LIVE block) and (c) a GrxModel descriptor whose pointers address the live block for the named tables and their records
// and the shared model for everything else; gravity lives in the descriptor itself.  A commit validates a world's stage rows, copies them to the live block and refills the
// private records from it; a world that breaks a rule keeps its live block and descriptor as they are.  The step kernels never read the stage rows.
//
// The meaning is that of writing the same MjModel fields in place without mj_setConst: whatever the compiler derived from them (dof_invweight0, geom_invweight0,
// eq_invweight, tendon_invweight0, meaninertia, the structural counts nfric / anydamp) keeps the nominal model's value.
#pragma once
#include "grx_engine.h"

// the tables that can be per world, in the order of their ids (GRX_PT_*); gravity (the three words of the descriptor) follows them
#define GRX_PARAM_TABLES(X) \
  X(body_mass) X(body_inertia) X(dof_damping) X(dof_armature) X(dof_frictionloss) X(jnt_stiffness) X(jnt_springref) X(jnt_range) X(act_gear) X(act_gainprm) X(act_biasprm) \
  X(act_ctrlrange) X(act_forcerange) X(pair_friction) X(pair_solref) X(pair_solimp)
enum {
#define X(n) GRX_PT_##n,
  GRX_PARAM_TABLES(X)
#undef X
  GRX_PT_gravity, GRX_NPT };
// the float record kinds that depend on one of them (recf_body depends on none: body_mass / body_inertia are read from the tables)
enum { GRX_PR_DOF = 0, GRX_PR_MPAIR, GRX_PR_JNT, GRX_PR_ACT, GRX_PR_PAIR, GRX_NPR };
// record kinds gathered from table t, as a bit set
GRX_HD int grx_param_record_deps(int t) {
  switch (t) {
    case GRX_PT_dof_damping: case GRX_PT_dof_frictionloss: case GRX_PT_jnt_stiffness: case GRX_PT_jnt_springref: return 1 << GRX_PR_DOF;
    case GRX_PT_dof_armature: return (1 << GRX_PR_DOF) | (1 << GRX_PR_MPAIR);
    case GRX_PT_jnt_range: return 1 << GRX_PR_JNT;
    case GRX_PT_act_gear: case GRX_PT_act_gainprm: case GRX_PT_act_biasprm: case GRX_PT_act_ctrlrange: case GRX_PT_act_forcerange: return 1 << GRX_PR_ACT;
    case GRX_PT_pair_friction: case GRX_PT_pair_solref: case GRX_PT_pair_solimp: return 1 << GRX_PR_PAIR;
    default: return 0;
  }
}
// bits of params_invalid (include/grx_capi.h GRX_PARAM_BAD_*)
enum { GRX_PB_NONFINITE = 1, GRX_PB_FRICTIONLOSS = 2, GRX_PB_DAMPING = 4, GRX_PB_INERTIAL = 8, GRX_PB_ARMATURE = 16, GRX_PB_JNT_RANGE = 32, GRX_PB_ACT_RANGE = 64 };

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// Record fills: ONE record's float words from the tables of h, in the field order and `float` arithmetic of grx_build_records (csrc/grx_host_model.h), so that a record
// filled from the nominal tables is bit for bit the shared one.  F addresses the record; its padding words are never written (they are zero from allocation on).
GRX_HD void grx_fill_prm(float* P, const float* solref, const float* solimp, float margin, float dA, float aux) {
  P[GRX_PRM_SOLREF] = solref[0]; P[GRX_PRM_SOLREF + 1] = solref[1];
  for (int k = 0; k < 5; k++) P[GRX_PRM_SOLIMP + k] = solimp[k];
  P[GRX_PRM_MARGIN] = margin; P[GRX_PRM_DA] = dA; P[GRX_PRM_AUX] = aux;
}
GRX_HD void grx_fill_recf_dof(const GrxModel& h, int q, int has_dofprm, float* F) {
  const int j = h.dof_jntid[q];
  F[0] = h.dof_damping[q]; F[1] = h.jnt_stiffness[j]; F[2] = h.jnt_springref[j]; F[3] = h.dof_armature[q];
  if (has_dofprm) grx_fill_prm(F + 4, h.dof_solref + 2 * q, h.dof_solimp + 5 * q, 0.0f, h.dof_invweight0[q], h.dof_frictionloss[q]);
}
GRX_HD void grx_fill_recf_mpair(const GrxModel& h, int e, float* F) { F[0] = h.dof_armature[h.mpair_i[e]]; }
GRX_HD void grx_fill_recf_jnt(const GrxModel& h, int j, float* F) {
  const int da = h.jnt_dofadr[j], qa = h.jnt_qposadr[j];
  for (int k = 0; k < 3; k++) { F[k] = h.jnt_pos[3 * j + k]; F[4 + k] = h.jnt_axis[3 * j + k]; }
  F[3] = h.qpos0[qa]; F[8] = h.jnt_range[2 * j]; F[9] = h.jnt_range[2 * j + 1];
  grx_fill_prm(F + 12, h.jnt_solref + 2 * j, h.jnt_solimp + 5 * j, h.jnt_margin[j], h.dof_invweight0[da], 0.0f);
}
GRX_HD void grx_fill_recf_act(const GrxModel& h, int a, float* F) {
  F[0] = h.act_gear[a]; F[1] = h.act_ctrlrange[2 * a]; F[2] = h.act_ctrlrange[2 * a + 1];
  for (int k = 0; k < 3; k++) { F[3 + k] = h.act_gainprm[3 * a + k]; F[6 + k] = h.act_biasprm[3 * a + k]; }
  F[9] = h.act_forcerange[2 * a]; F[10] = h.act_forcerange[2 * a + 1];
}
GRX_HD void grx_fill_recf_pair(const GrxModel& h, int p, float* F) {
  const int g1 = h.pair_geom1[p], g2 = h.pair_geom2[p];
  F[0] = h.pair_margin[p]; F[1] = h.pair_gap[p]; F[2] = h.pair_margin[p] - h.pair_gap[p];
  for (int k = 0; k < 5; k++) F[3 + k] = h.pair_friction[5 * p + k];
  const float tran = h.geom_invweight0[2 * g1] + h.geom_invweight0[2 * g2];
  grx_fill_prm(F + 8, h.pair_solref + 2 * p, h.pair_solimp + 5 * p, F[2], tran, h.pair_friction[5 * p]);
  F[8 + GRX_PRM_DA2] = (float)h.pair_condim[p];
  for (int k = 0; k < 3; k++) { F[20 + k] = h.geom_size[3 * g1 + k]; F[24 + k] = h.geom_size[3 * g2 + k]; }
}
// entities and words per record of a kind
struct GrxParamCounts { int n[GRX_NPR]; int has_dofprm; };
GRX_HD int grx_param_record_words(int kind) { return kind == GRX_PR_DOF ? GRX_RDF : kind == GRX_PR_MPAIR ? 1 : kind == GRX_PR_JNT ? GRX_RJF : kind == GRX_PR_ACT ? GRX_RAF : GRX_RPF; }
// record e of `kind` of the model view h, written where h's own record pointer says (the descriptor's private region)
GRX_HD void grx_fill_record(const GrxModel& h, int kind, int e, int has_dofprm) {
  switch (kind) {
    case GRX_PR_DOF: grx_fill_recf_dof(h, e, has_dofprm, const_cast<float*>(h.recf_dof) + GRX_RDF * e); break;
    case GRX_PR_MPAIR: grx_fill_recf_mpair(h, e, const_cast<float*>(h.recf_mpair) + e); break;
    case GRX_PR_JNT: grx_fill_recf_jnt(h, e, const_cast<float*>(h.recf_jnt) + GRX_RJF * e); break;
    case GRX_PR_ACT: grx_fill_recf_act(h, e, const_cast<float*>(h.recf_act) + GRX_RAF * e); break;
    default: grx_fill_recf_pair(h, e, const_cast<float*>(h.recf_pair) + GRX_RPF * e); break;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// The rules of a commit, for one element i of table t: v the staged value, v2 its partner where the rule spans two words (a range's upper end), nom the nominal value.
GRX_HD int grx_param_check(int t, float v, float v2, float nom, int anydamp, int limited) {
  int bits = (v == v && fabsf(v) <= 3.402823466e38f) ? 0 : GRX_PB_NONFINITE;
  switch (t) {
    case GRX_PT_dof_frictionloss: if ((v > 0.0f) != (nom > 0.0f)) bits |= GRX_PB_FRICTIONLOSS; break;   // nfric sizes the row tables
    case GRX_PT_dof_damping: if (!(v >= 0.0f) || (!anydamp && v != 0.0f)) bits |= GRX_PB_DAMPING; break;
    case GRX_PT_body_mass: case GRX_PT_body_inertia: if (nom > 0.0f && !(v > 0.0f)) bits |= GRX_PB_INERTIAL; break;
    case GRX_PT_dof_armature: if (!(v >= 0.0f)) bits |= GRX_PB_ARMATURE; break;
    case GRX_PT_jnt_range: if (limited && !(v < v2)) bits |= GRX_PB_JNT_RANGE; break;
    case GRX_PT_act_ctrlrange: case GRX_PT_act_forcerange: if (!(v <= v2)) bits |= GRX_PB_ACT_RANGE; break;
    default: break;
  }
  return bits;
}

// what the commit kernels take by value
struct GrxParamCommit {
  const float* stage[GRX_NPT];     // [N, cnt[t]] or null (not named)
  const float* nominal[GRX_NPT];   // the shared model's table (device), null for gravity
  int cnt[GRX_NPT], live_off[GRX_NPT];   // words of a row; its offset inside a world's live block
  float* live; int stride;         // [N, stride]
  GrxModel* desc; GrxModel* desc_large;   // [N] each; desc_large null without a large-table handle
  const int* jnt_limited;          // the shared model's table
  int anydamp, kinds;              // kinds: bit set of the record kinds with a private copy
  GrxParamCounts counts;
  const unsigned char* mask;       // [N] or null
  int* bits; int* bits_out;        // [N] the object's own row; the caller's row or null
  int n_worlds;
};

#if !defined(GRX_EMU)
// first commit kernel, one wave per world: validate the stage rows; a clean world's rows go to its live block and its gravity into its descriptor(s)
__device__ __forceinline__ void grx_param_commit_rows(const GrxParamCommit& a, int w, int lane_) {
  if (w >= a.n_worlds) return;
  if (a.mask && !a.mask[w]) return;
  int bits = 0;
  for (int t = 0; t < GRX_NPT; t++) {
    if (!a.stage[t]) continue;
    const int n = a.cnt[t];
    const float* row = a.stage[t] + (size_t)w * n;
    const bool pairwise = t == GRX_PT_jnt_range || t == GRX_PT_act_ctrlrange || t == GRX_PT_act_forcerange;
    for (int i = lane_; i < n; i += 64) {
      const float v = row[i], nom = a.nominal[t] ? a.nominal[t][i] : 0.0f;
      const float v2 = (pairwise && !(i & 1) && i + 1 < n) ? row[i + 1] : v;
      const int t_eff = (pairwise && (i & 1)) ? GRX_PT_gravity : t;      // the upper end of a range is checked with its lower end; on its own only for finiteness
      bits |= grx_param_check(t_eff, v, v2, nom, a.anydamp, t == GRX_PT_jnt_range ? a.jnt_limited[i >> 1] : 0);
    }
  }
  for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
  if (lane_ == 0) { a.bits[w] = bits; if (a.bits_out) a.bits_out[w] = bits; }
  if (bits) return;
  float* live = a.live + (size_t)w * a.stride;
  for (int t = 0; t < GRX_NPT; t++) {
    if (!a.stage[t]) continue;
    const int n = a.cnt[t];
    const float* row = a.stage[t] + (size_t)w * n;
    if (t == GRX_PT_gravity) {
      if (lane_ < 3) { a.desc[w].gravity[lane_] = row[lane_]; if (a.desc_large) a.desc_large[w].gravity[lane_] = row[lane_]; }
    } else {
      for (int i = lane_; i < n; i += 64) live[a.live_off[t] + i] = row[i];
    }
  }
}
// second commit kernel (behind the first on the stream), one wave per world: refill the private records of the worlds the first one accepted, lanes over entities, from the
// world's own descriptor -- the tables as the step kernels will see them
__device__ __forceinline__ void grx_param_commit_records(const GrxParamCommit& a, int w, int lane_) {
  if (w >= a.n_worlds) return;
  if (a.mask && !a.mask[w]) return;
  if (a.bits[w]) return;
  const GrxModel& h = a.desc[w];
  for (int kind = 0; kind < GRX_NPR; kind++) {
    if (!((a.kinds >> kind) & 1)) continue;
    for (int e = lane_; e < a.counts.n[kind]; e += 64) grx_fill_record(h, kind, e, a.counts.has_dofprm);
  }
}
#endif
