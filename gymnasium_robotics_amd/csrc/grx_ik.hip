// grx_ik.hip -- the inverse-kinematics kernel of the task-free stepper (include/grx_capi.h grx_sim_ik), a translation unit of its own: it shares no code with the step kernels
// and is linked into libgrx_hip.so behind the units of grx_kernels.hip, whose C ABI checks the arguments and calls grx_tu_ik_launch.
//
// SHAPE ("Inverse kinematics").  The whole damped-least-squares loop of a world -- kinematics, error, Jacobian, J J' + damping^2 I, Cholesky, J' y, integration --
// runs in ONE wave, four worlds per 256-thread workgroup.  The work is small and serial in its stages, so it is latency that counts: everything between the first load of
// qpos0 and the last store of qpos stays in LDS and registers.  The workgroup stages the model's kinematic tables, the site records and their chain masks once for its four
// waves; each wave then owns a slice (q, body frames, joint anchors / axes, J [m][nv], the m x m system) and synchronises with ITSELF only (IK_SYNC: a wave barrier and an LDS
// fence), so a wave whose world has converged leaves the loop at once and its SIMD goes to the next workgroup's waves.  No matrix instruction: the largest product is
// 24 x nv x 24 per world.
#include <hip/hip_runtime.h>

#include "grx_ik.h"

// a wave's own writes to its LDS slice become visible to its own lanes: LDS serves a wave's instructions in order, so what is needed is that the compiler neither moves an
// access across this point nor lets the lanes drift apart; the fence also waits for the outstanding LDS operations
#define IK_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)
#define IK_PICK(arr, k) ((k) == 0 ? (arr)[0] : (k) == 1 ? (arr)[1] : (k) == 2 ? (arr)[2] : (arr)[3])      // the argument block lives in scalar registers: no dynamic index

static __device__ __forceinline__ void ik_rot(float* o, const float* v, const float* q) {      // o = R(q) v, q unit
  const float tx = 2.0f * (q[2] * v[2] - q[3] * v[1]), ty = 2.0f * (q[3] * v[0] - q[1] * v[2]), tz = 2.0f * (q[1] * v[1] - q[2] * v[0]);
  o[0] = v[0] + q[0] * tx + (q[2] * tz - q[3] * ty);
  o[1] = v[1] + q[0] * ty + (q[3] * tx - q[1] * tz);
  o[2] = v[2] + q[0] * tz + (q[1] * ty - q[2] * tx);
}
static __device__ __forceinline__ void ik_mulq(float* o, const float* a, const float* b) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
static __device__ __forceinline__ void ik_norm4(float* q) {      // mju_normalize4: a zero quaternion becomes the identity
  const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < 1e-15f) { q[0] = 1.0f; q[1] = q[2] = q[3] = 0.0f; return; }
  const float s = 1.0f / n;
  q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
}
static __device__ __forceinline__ float ik_wave_sum(float v) {      // a butterfly: every lane ends with the same bits
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
static __device__ __forceinline__ bool ik_finite(float v) { return fabsf(v) <= 3.4028235e38f; }

extern "C" __global__ void __launch_bounds__(64 * GRX_IK_WAVES)
grx_ik_kernel(GrxIkArgs a) {
  extern __shared__ float lds[];
  const GrxIkLayout L = grx_ik_layout(a.nq, a.nv, a.nbody, a.njnt, a.nlevel, a.n_sites, a.rot);
  const int nq = a.nq, nv = a.nv, nb = a.nbody, nj = a.njnt, K = a.n_sites, m = L.m, ldj = L.ldj, lda = L.lda, rows = a.rot ? 6 : 3;
  int* bI = (int*)(lds + L.b_int); float* bF = lds + L.b_flt;        // body: parent, jntadr, jntnum, mocapid | pos 3, quat 4
  int* jI = (int*)(lds + L.j_int); float* jF = lds + L.j_flt;        // joint: type, qposadr, dofadr, bodyid, limited | pos 3, axis 3, range 2
  int* dJ = (int*)(lds + L.d_jnt); float* q0 = lds + L.q0;
  int* order = (int*)(lds + L.order); int* level = (int*)(lds + L.level);
  int* sI = (int*)(lds + L.s_int); float* sF = lds + L.s_flt;
  {
    const int t = threadIdx.x, nt = blockDim.x;
    for (int b = t; b < nb; b += nt) {
      bI[4 * b] = a.body_parent[b]; bI[4 * b + 1] = a.body_jntadr[b]; bI[4 * b + 2] = a.body_jntnum[b]; bI[4 * b + 3] = a.body_mocapid[b];
      for (int c = 0; c < 3; c++) bF[7 * b + c] = a.body_pos[3 * b + c];
      for (int c = 0; c < 4; c++) bF[7 * b + 3 + c] = a.body_quat[4 * b + c];
    }
    for (int j = t; j < nj; j += nt) {
      jI[5 * j] = a.jnt_type[j]; jI[5 * j + 1] = a.jnt_qposadr[j]; jI[5 * j + 2] = a.jnt_dofadr[j]; jI[5 * j + 3] = a.jnt_bodyid[j]; jI[5 * j + 4] = a.jnt_limited[j];
      for (int c = 0; c < 3; c++) { jF[8 * j + c] = a.jnt_pos[3 * j + c]; jF[8 * j + 3 + c] = a.jnt_axis[3 * j + c]; }
      jF[8 * j + 6] = a.jnt_range[2 * j]; jF[8 * j + 7] = a.jnt_range[2 * j + 1];
    }
    for (int d = t; d < nv; d += nt) dJ[d] = a.dof_jntid[d];
    for (int i = t; i < nq; i += nt) q0[i] = a.qpos0[i];
    for (int i = t; i < nb - 1; i += nt) order[i] = a.body_order[i];
    for (int i = t; i < a.nlevel + 2; i += nt) level[i] = a.level_adr[i];
    if (t < K) {
      const int s = IK_PICK(a.site, t);
      sI[3 * t] = IK_PICK(a.site_body, t); sI[3 * t + 1] = (int)IK_PICK(a.chain_lo, t); sI[3 * t + 2] = (int)IK_PICK(a.chain_hi, t);
      for (int c = 0; c < 3; c++) sF[7 * t + c] = a.site_pos[3 * s + c];
      for (int c = 0; c < 4; c++) sF[7 * t + 3 + c] = a.site_quat[4 * s + c];
    }
  }
  __syncthreads();      // the only workgroup barrier: from here on a wave reads the tables and its own slice
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, world = blockIdx.x * a.wpb + wv;
  if (world >= a.n_worlds) return;
  float* S = lds + L.tables + wv * L.slice;
  float *Q = S + L.q, *XP = S + L.xpos, *XQ = S + L.xquat, *AN = S + L.anchor, *AX = S + L.axis, *SP = S + L.spos, *T = S + L.tgt, *E = S + L.e, *Jm = S + L.J, *A = S + L.A,
        *Y = S + L.y, *DQ = S + L.dq;
  const float* qin = a.qstart + (size_t)world * nq;
  float* qout = a.qpos + (size_t)world * nq;
  if (a.mask && !a.mask[world]) {
    for (int i = lane; i < nq; i += 64) qout[i] = qin[i];
    if (lane == 0) { a.err[world] = -1.0f; a.iters[world] = 0; }
    return;
  }
  bool bad = false;
  for (int i = lane; i < nq; i += 64) { const float v = qin[i]; Q[i] = v; bad |= !ik_finite(v); }
  for (int i = lane; i < 3 * K; i += 64) { const float v = a.target_pos[(size_t)world * 3 * K + i]; T[7 * (i / 3) + i % 3] = v; bad |= !ik_finite(v); }
  if (a.rot) for (int i = lane; i < 4 * K; i += 64) { const float v = a.target_quat[(size_t)world * 4 * K + i]; T[7 * (i / 4) + 3 + i % 4] = v; bad |= !ik_finite(v); }
  if (__any(bad)) {      // non-finite start or target: the world's row comes back as given
    for (int i = lane; i < nq; i += 64) qout[i] = qin[i];
    if (lane == 0) { a.err[world] = __builtin_inff(); a.iters[world] = 0; }
    return;
  }
  IK_SYNC();
  const float* mpos = a.mocap_pos + (size_t)world * 3 * a.nmocap;
  const float* mquat = a.mocap_quat + (size_t)world * 4 * a.nmocap;
  int it = 0;
  float errn = 0.0f;
  for (;;) {
    // ---- 1. kinematics.  lane = body: its pose in the parent's frame, its joints' anchors and axes in that frame (the trigonometry of every body at once)
    for (int b = lane; b < nb; b += 64) {
      float p[3] = {0.0f, 0.0f, 0.0f}, q[4] = {1.0f, 0.0f, 0.0f, 0.0f};
      if (b > 0) {
        const int ja = bI[4 * b + 1], jn = bI[4 * b + 2], mid = bI[4 * b + 3];
        for (int c = 0; c < 3; c++) p[c] = bF[7 * b + c];
        for (int c = 0; c < 4; c++) q[c] = bF[7 * b + 3 + c];
        if (mid >= 0) {
          for (int c = 0; c < 3; c++) p[c] = mpos[3 * mid + c];
          for (int c = 0; c < 4; c++) q[c] = mquat[4 * mid + c];
          ik_norm4(q);
        } else if (jn == 1 && jI[5 * ja] == 0) {      // a free joint: qpos is the world pose
          const int qa = jI[5 * ja + 1];
          for (int c = 0; c < 3; c++) p[c] = Q[qa + c];
          for (int c = 0; c < 4; c++) q[c] = Q[qa + 3 + c];
          ik_norm4(q);
          for (int c = 0; c < 3; c++) { AN[3 * ja + c] = p[c]; AX[3 * ja + c] = c == 2 ? 1.0f : 0.0f; }
        } else {
          for (int k = 0; k < jn; k++) {
            const int j = ja + k, jt = jI[5 * j], qa = jI[5 * j + 1];
            const float jp[3] = {jF[8 * j], jF[8 * j + 1], jF[8 * j + 2]}, jx[3] = {jF[8 * j + 3], jF[8 * j + 4], jF[8 * j + 5]};
            float an[3], ax[3];
            ik_rot(an, jp, q); ik_rot(ax, jx, q);
            for (int c = 0; c < 3; c++) { an[c] += p[c]; AN[3 * j + c] = an[c]; AX[3 * j + c] = ax[c]; }
            const float dq = Q[qa] - q0[qa];
            if (jt == 2) {
              for (int c = 0; c < 3; c++) p[c] += ax[c] * dq;
            } else if (jt == 3) {
              float sn, cs;
              sincosf(0.5f * dq, &sn, &cs);
              const float qr[4] = {cs, jx[0] * sn, jx[1] * sn, jx[2] * sn};
              float qn[4], off[3];
              ik_mulq(qn, q, qr); ik_norm4(qn);
              for (int c = 0; c < 4; c++) q[c] = qn[c];
              ik_rot(off, jp, q);
              for (int c = 0; c < 3; c++) p[c] = an[c] - off[c];
            }
          }
        }
      }
      for (int c = 0; c < 3; c++) XP[3 * b + c] = p[c];
      for (int c = 0; c < 4; c++) XQ[4 * b + c] = q[c];
    }
    IK_SYNC();
    // the composition walks the depth levels (level 1 hangs from the world: nothing to compose); a level's bodies read finished parents
    for (int d = 2; d <= a.nlevel; d++) {
      const int i1 = level[d + 1];
      for (int i = level[d] + lane; i < i1; i += 64) {
        const int b = order[i], par = bI[4 * b];
        const float pq[4] = {XQ[4 * par], XQ[4 * par + 1], XQ[4 * par + 2], XQ[4 * par + 3]}, lp[3] = {XP[3 * b], XP[3 * b + 1], XP[3 * b + 2]},
                    lq[4] = {XQ[4 * b], XQ[4 * b + 1], XQ[4 * b + 2], XQ[4 * b + 3]};
        float v[3], qn[4];
        ik_rot(v, lp, pq); ik_mulq(qn, pq, lq); ik_norm4(qn);
        for (int c = 0; c < 3; c++) XP[3 * b + c] = XP[3 * par + c] + v[c];
        for (int c = 0; c < 4; c++) XQ[4 * b + c] = qn[c];
      }
      IK_SYNC();
    }
    // joint anchors and axes to the world frame (a free joint's already are), the sites, and 2. the error
    for (int j = lane; j < nj; j += 64) {
      const int par = bI[4 * jI[5 * j + 3]];
      if (jI[5 * j] == 0 || par <= 0) continue;
      const float pq[4] = {XQ[4 * par], XQ[4 * par + 1], XQ[4 * par + 2], XQ[4 * par + 3]}, an[3] = {AN[3 * j], AN[3 * j + 1], AN[3 * j + 2]}, ax[3] = {AX[3 * j], AX[3 * j + 1], AX[3 * j + 2]};
      float wa[3], wx[3];
      ik_rot(wa, an, pq); ik_rot(wx, ax, pq);
      for (int c = 0; c < 3; c++) { AN[3 * j + c] = wa[c] + XP[3 * par + c]; AX[3 * j + c] = wx[c]; }
    }
    if (lane < K) {
      const int k = lane, b = sI[3 * k], base = rows * k;
      const float bq[4] = {XQ[4 * b], XQ[4 * b + 1], XQ[4 * b + 2], XQ[4 * b + 3]}, lp[3] = {sF[7 * k], sF[7 * k + 1], sF[7 * k + 2]};
      float sp[3];
      ik_rot(sp, lp, bq);
      for (int c = 0; c < 3; c++) { sp[c] += XP[3 * b + c]; SP[3 * k + c] = sp[c]; E[base + c] = T[7 * k + c] - sp[c]; }
      if (a.rot) {
        const float lq[4] = {sF[7 * k + 3], sF[7 * k + 4], sF[7 * k + 5], sF[7 * k + 6]}, tq[4] = {T[7 * k + 3], T[7 * k + 4], T[7 * k + 5], T[7 * k + 6]};
        float sq[4], d[4];
        ik_mulq(sq, bq, lq);
        const float cj[4] = {sq[0], -sq[1], -sq[2], -sq[3]};
        ik_mulq(d, tq, cj);
        if (d[0] < 0.0f) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; d[3] = -d[3]; }
        const float vn = sqrtf(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
        const float s = vn > 0.0f ? a.rot_weight * 2.0f * atan2f(vn, d[0]) / vn : 0.0f;
        for (int c = 0; c < 3; c++) E[base + 3 + c] = s * d[1 + c];
      }
    }
    IK_SYNC();
    {
      const float v = lane < m ? E[lane] : 0.0f;
      errn = sqrtf(ik_wave_sum(v * v));
    }
    // ---- 3. converged, or out of updates (wave-uniform: errn holds the same bits in every lane)
    if (errn < a.tol || it >= a.max_iters) break;
    // ---- 4. the Jacobian, lane = dof: its column of every site's rows, zero where the dof is not in the site's chain or not the call's to move
    for (int d = lane; d < nv; d += 64) {
      const int j = dJ[d], jt = jI[5 * j], i = d - jI[5 * j + 2], b = jI[5 * j + 3];
      float ax[3] = {AX[3 * j], AX[3 * j + 1], AX[3 * j + 2]}, ref[3] = {AN[3 * j], AN[3 * j + 1], AN[3 * j + 2]};
      bool lin = jt == 2;
      if (jt == 0) {
        const float u[3] = {(i % 3) == 0 ? 1.0f : 0.0f, (i % 3) == 1 ? 1.0f : 0.0f, (i % 3) == 2 ? 1.0f : 0.0f};
        if (i < 3) { lin = true; ax[0] = u[0]; ax[1] = u[1]; ax[2] = u[2]; }
        else {      // a rotational dof of a free joint turns about a body axis, through the body's origin
          const float bq[4] = {XQ[4 * b], XQ[4 * b + 1], XQ[4 * b + 2], XQ[4 * b + 3]};
          ik_rot(ax, u, bq);
          for (int c = 0; c < 3; c++) ref[c] = XP[3 * b + c];
        }
      }
      for (int k = 0; k < K; k++) {
        const unsigned word = (unsigned)(d < 32 ? sI[3 * k + 1] : sI[3 * k + 2]);
        const bool on = d < 64 && ((word >> (d & 31)) & 1u);
        const float r[3] = {SP[3 * k] - ref[0], SP[3 * k + 1] - ref[1], SP[3 * k + 2] - ref[2]};
        float jp[3] = {ax[1] * r[2] - ax[2] * r[1], ax[2] * r[0] - ax[0] * r[2], ax[0] * r[1] - ax[1] * r[0]};
        if (lin) { jp[0] = ax[0]; jp[1] = ax[1]; jp[2] = ax[2]; }
        const int base = rows * k;
        for (int c = 0; c < 3; c++) Jm[(base + c) * ldj + d] = on ? jp[c] : 0.0f;
        if (a.rot) for (int c = 0; c < 3; c++) Jm[(base + 3 + c) * ldj + d] = (on && !lin) ? a.rot_weight * ax[c] : 0.0f;
      }
    }
    IK_SYNC();
    // ---- 5. A = J J' + damping^2 I: the lower triangle's m (m + 1) / 2 entries over the lanes, each a serial dot over nv
    for (int idx = lane; idx < m * (m + 1) / 2; idx += 64) {
      int r = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
      while (r * (r + 1) / 2 > idx) r--;
      while ((r + 1) * (r + 2) / 2 <= idx) r++;
      const int c = idx - r * (r + 1) / 2;
      float s = r == c ? a.damping2 : 0.0f;
      for (int d = 0; d < nv; d++) s += Jm[r * ldj + d] * Jm[c * ldj + d];
      A[r * lda + c] = s;
    }
    IK_SYNC();
    // Cholesky, left-looking, lane = row: column c of L from the columns before it; the pivot goes round by a lane read
    for (int c = 0; c < m; c++) {
      float s = 1.0f;
      const bool mine = lane >= c && lane < m;
      if (mine) {
        s = A[lane * lda + c];
        for (int k = 0; k < c; k++) s -= A[lane * lda + k] * A[c * lda + k];
      }
      const float piv = sqrtf(fmaxf(__shfl(s, c, 64), 1e-30f));
      if (mine) A[lane * lda + c] = lane == c ? piv : s / piv;
      IK_SYNC();
    }
    // L z = e, then L' y = z: each lane carries its row's residual in a register, the solved component goes round by a lane read
    {
      float r = lane < m ? E[lane] : 0.0f, z = 0.0f, y = 0.0f;
      for (int c = 0; c < m; c++) {
        const float zc = __shfl(r, c, 64) / A[c * lda + c];
        if (lane == c) z = zc;
        if (lane > c && lane < m) r -= A[lane * lda + c] * zc;
      }
      r = z;
      for (int c = m - 1; c >= 0; c--) {
        const float yc = __shfl(r, c, 64) / A[c * lda + c];
        if (lane == c) y = yc;
        if (lane < c) r -= A[c * lda + lane] * yc;
      }
      if (lane < m) Y[lane] = y;
    }
    IK_SYNC();
    // dq = J' y, lane = dof, scaled to max_step
    float n2 = 0.0f;
    for (int d = lane; d < nv; d += 64) {
      float s = 0.0f;
      for (int r = 0; r < m; r++) s += Jm[r * ldj + d] * Y[r];
      DQ[d] = s;
      n2 += s * s;
    }
    const float nrm = sqrtf(ik_wave_sum(n2)), sc = nrm > a.max_step ? a.max_step / nrm : 1.0f;
    IK_SYNC();
    // ---- 6. q <- mj_integratePos(q, dq, 1), lane = joint; a coordinate whose dof the call may not move keeps its bits
    for (int j = lane; j < nj; j += 64) {
      const int jt = jI[5 * j], qa = jI[5 * j + 1], da = jI[5 * j + 2];
      const unsigned long long sel = ((unsigned long long)a.dofsel[1] << 32) | a.dofsel[0];
      if (jt == 0) {
        if (!((sel >> da) & 0x3full)) continue;
        for (int c = 0; c < 3; c++) Q[qa + c] += sc * DQ[da + c];
        const float v[3] = {sc * DQ[da + 3], sc * DQ[da + 4], sc * DQ[da + 5]}, ang = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        float q[4] = {Q[qa + 3], Q[qa + 4], Q[qa + 5], Q[qa + 6]}, qn[4] = {q[0], q[1], q[2], q[3]};
        if (ang > 1e-15f) {
          float sn, cs;
          sincosf(0.5f * ang, &sn, &cs);
          const float qr[4] = {cs, v[0] / ang * sn, v[1] / ang * sn, v[2] / ang * sn};
          ik_mulq(qn, q, qr);
        }
        ik_norm4(qn);
        for (int c = 0; c < 4; c++) Q[qa + 3 + c] = qn[c];
      } else if ((sel >> da) & 1ull) {
        float x = Q[qa] + sc * DQ[da];
        if (a.clamp_limits && jI[5 * j + 4]) x = fminf(fmaxf(x, jF[8 * j + 6]), jF[8 * j + 7]);
        Q[qa] = x;
      }
    }
    IK_SYNC();
    it++;
  }
  for (int i = lane; i < nq; i += 64) qout[i] = Q[i];
  if (lane == 0) { a.err[world] = errn; a.iters[world] = it; }
}

// worlds per workgroup: four, or as many as fit the LDS a workgroup may ask for; 0: not even one world fits
extern "C" int grx_tu_ik_wpb(const GrxIkArgs* a, int* bytes) {
  const GrxIkLayout L = grx_ik_layout(a->nq, a->nv, a->nbody, a->njnt, a->nlevel, a->n_sites, a->rot);
  int wpb = GRX_IK_WAVES;
  while (wpb > 0 && 4ll * ((long long)L.tables + (long long)wpb * L.slice) > GRX_IK_LDS_BYTES) wpb >>= 1;
  if (bytes) *bytes = 4 * (L.tables + (wpb > 0 ? wpb : 1) * L.slice);
  return wpb;
}

extern "C" int grx_tu_ik_launch(const GrxIkArgs* a, void* stream) {
  int bytes = 0;
  GrxIkArgs k = *a;
  k.wpb = grx_tu_ik_wpb(a, &bytes);
  if (k.wpb < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(grx_ik_kernel, dim3((unsigned)((k.n_worlds + k.wpb - 1) / k.wpb)), dim3(64u * (unsigned)k.wpb), (size_t)bytes, (hipStream_t)stream, k);
  return (int)hipGetLastError();
}
