// grx_ik.h -- what the inverse-kinematics kernel (csrc/grx_ik.hip) and its C ABI (csrc/grx_ik_api.h, include/grx_capi.h grx_sim_ik) share: the launch's argument block and the
// LDS layout of a workgroup.  A header of its own, outside the engine template, as grx_rays.h is.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GRX_IK_FN __host__ __device__ static inline
#else
#define GRX_IK_FN static inline
#endif

#define GRX_IK_MAXSITE 4            // sites per call: the error has at most 6 * 4 = 24 components, one lane each in the factorisation
#define GRX_IK_WAVES 4              // worlds (= waves) of a full workgroup
#define GRX_IK_LDS_BYTES 65536      // what a workgroup may ask for without raising the kernel's limit: a launch that needs more per world takes fewer worlds per workgroup

struct GrxIkArgs {
  // the model's kinematic tables (device, fp32 / int32: include/grx_model_fields.def)
  const int *body_parent, *body_jntadr, *body_jntnum, *body_mocapid, *jnt_type, *jnt_qposadr, *jnt_dofadr, *jnt_bodyid, *jnt_limited, *dof_jntid, *body_order, *level_adr;
  const float *body_pos, *body_quat, *jnt_pos, *jnt_axis, *jnt_range, *qpos0, *site_pos, *site_quat;
  int nq, nv, nbody, njnt, nmocap, nlevel;      // nlevel = maxdepth: level_adr has nlevel + 2 entries, level d = body_order[level_adr[d] .. level_adr[d + 1])
  // the call
  const float *qstart, *mocap_pos, *mocap_quat, *target_pos, *target_quat;      // [N,nq] [N,nmocap,3] [N,nmocap,4] [N,K,3] [N,K,4] (target_quat NULL: positions only)
  const unsigned char* mask;
  float* qpos; float* err; int* iters;
  int site[GRX_IK_MAXSITE], site_body[GRX_IK_MAXSITE];
  unsigned chain_lo[GRX_IK_MAXSITE], chain_hi[GRX_IK_MAXSITE];   // per site: the dofs of its body's chain that the call may move (64 bits: a model handle has at most 64 dofs)
  unsigned dofsel[2];                  // the dofs the call may move
  int n_sites, rot, max_iters, clamp_limits;
  float damping2, max_step, tol, rot_weight;
  int n_worlds, wpb;                   // worlds per workgroup (1, 2 or 4)
};

// LDS of a workgroup, in 32-bit words: the tables all its waves read, then one slice per wave
struct GrxIkLayout {
  // tables
  int b_int, b_flt, j_int, j_flt, d_jnt, q0, order, level, s_int, s_flt, tables;      // body ints [4 nbody], body floats [7 nbody], joint ints [5 njnt], joint floats [8 njnt], ...
  // slice (offsets from the slice's first word)
  int q, xpos, xquat, anchor, axis, spos, tgt, e, J, A, y, dq, slice;
  int ldj, lda, m;
};
GRX_IK_FN GrxIkLayout grx_ik_layout(int nq, int nv, int nbody, int njnt, int nlevel, int n_sites, int rot) {
  GrxIkLayout L;
  int p = 0;
  L.b_int = p; p += 4 * nbody;
  L.b_flt = p; p += 7 * nbody;
  L.j_int = p; p += 5 * njnt;
  L.j_flt = p; p += 8 * njnt;
  L.d_jnt = p; p += nv;
  L.q0 = p; p += nq;
  L.order = p; p += nbody;
  L.level = p; p += nlevel + 2;
  L.s_int = p; p += 3 * n_sites;      // per site: its body, the two words of its chain mask
  L.s_flt = p; p += 7 * n_sites;      // per site: pos, quat in that body's frame
  L.tables = p;
  L.m = (rot ? 6 : 3) * n_sites;
  L.ldj = nv | 1;          // odd row strides: the lanes that read one column of different rows hit different banks
  L.lda = L.m | 1;
  p = 0;
  L.q = p; p += nq;
  L.xpos = p; p += 3 * nbody;
  L.xquat = p; p += 4 * nbody;
  L.anchor = p; p += 3 * njnt;
  L.axis = p; p += 3 * njnt;
  L.spos = p; p += 3 * n_sites;
  L.tgt = p; p += 7 * n_sites;
  L.e = p; p += L.m;
  L.J = p; p += L.m * L.ldj;
  L.A = p; p += L.m * L.lda;
  L.y = p; p += L.m;
  L.dq = p; p += nv;
  L.slice = p;
  return L;
}
