// grx_camera_rgb.hip -- the shading render kernel of the task-free stepper's colour / surface-normal cameras (include/grx_capi.h grx_sim_render_rgb), a translation unit of
// its own next to grx_camera.hip: it shares the staged geom record and the hit routines of csrc/grx_rays.h and the binning rule of csrc/grx_camera.h with the depth kernel,
// takes the normal routines and the colour rule from csrc/grx_shade.h, and leaves the depth kernel's code object what it is.
//
// SHAPE ("Cameras").  STAGE, BIN and TRACE are those of grx_camera.hip, statement for statement, so depth and seg come out bit for bit: one workgroup of 256
// threads per (world, camera) image, the geoms binned to 8 x 8 (or 16 x 4) pixel tiles, a wave per tile, lane <-> pixel, the tile's mask words wave-uniform, ascending geom id.
// STAGE also puts the staged geoms' colours into LDS beside the records (one float3 per geom, clamped to [0, 1]; the world's own row with colors_per_world), loaded by the
// threads that stage the records.  What is new is a fourth phase:
//   SHADE  after TRACE the 64 lanes of a tile hold different winners, and a per-lane type switch in the normal routine would diverge seven ways.  So the wave walks its
//          DISTINCT winners: while a lane is unshaded it takes the winner g of the first such lane (readfirstlane); every lane whose winner is g computes its normal from
//          the staged record -- g is wave-uniform, so the record and the colour are LDS broadcasts and the type switch is a scalar branch -- shades, and leaves the loop.  A
//          tile sees few distinct geoms (that is what the binning established), so the loop is short.
// STORES.  rgba is packed RGBA8, one dword store per lane (a tile row of 8 pixels is one 32-byte segment); normal is three floats per lane.
// PASSES.  With more geoms than one pass stages, a lane shades in the pass that holds its current winner and stores then; a later pass stores again only where it found a
// nearer hit; the last pass writes the background / a zero normal where there is no hit (or one beyond max_dist).  A lane never reads its colour or normal back, and reads
// only its own earlier depth, as the depth kernel does.
#include <hip/hip_runtime.h>

#include "grx_shade.h"

template <int TW, int TH>
__device__ __forceinline__ void grx_camera_rgb_image(const GrxCamRgbArgs& s, float* stage, float* cols, int* rect, unsigned* masks, float* cam) {
  static_assert(TW * TH == 64, "a tile is a wave");
  const GrxCamArgs& a = s.c;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int world = blockIdx.x, k = blockIdx.y, H = a.height, W = a.width;
  const float* xpos = a.xpos + (size_t)world * a.nbody * 3;
  const float* xquat = a.xquat + (size_t)world * a.nbody * 4;
  const float* colors = s.colors ? s.colors + (s.colors_per_world ? (size_t)world * a.ngeom * 3 : 0) : nullptr;
  if (t == 0) {      // cam: origin 3, camera -> world matrix 9 (row-major), 1.0 if all of it is finite
    if (a.pose_pos) {
      const float* pp = a.pose_pos + ((size_t)world * a.n_cams + k) * 3;
      const float* pm = a.pose_mat + ((size_t)world * a.n_cams + k) * 9;
      for (int i = 0; i < 3; i++) cam[i] = pp[i];
      for (int i = 0; i < 9; i++) cam[3 + i] = pm[i];
    } else {      // x_body o (cam_pos, cam_quat): the record of a "geom" at the camera's place
      float rec[GRX_RAY_REC];
      const int zero = 0, body = a.cam_body[k];
      const float none[3] = {0.0f, 0.0f, 0.0f}, cp[3] = {a.cam_pos[k][0], a.cam_pos[k][1], a.cam_pos[k][2]}, cq[4] = {a.cam_quat[k][0], a.cam_quat[k][1], a.cam_quat[k][2], a.cam_quat[k][3]};
      grx_ray_stage(rec, 0, xpos, xquat, &zero, &body, cp, cq, none, none, nullptr, nullptr);
      for (int i = 0; i < 12; i++) cam[i] = rec[i];
    }
    bool ok = true;
    for (int i = 0; i < 12; i++) ok = ok && fabsf(cam[i]) < INFINITY;
    cam[12] = ok ? 1.0f : 0.0f;
  }
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH, ntile = tiles_x * tiles_y;
  const float ay = a.cam_tan[k], ax = ay * (float)W / (float)H;
  const int skip_a = a.exclude_body[k], skip_b = (a.exclude_own_body && !a.pose_pos) ? a.cam_body[k] : -1;
  const size_t image = ((size_t)world * a.n_cams + k) * (size_t)H * W;
  for (int g0 = 0; g0 == 0 || g0 < a.ngeom; g0 += GRX_CAM_STAGE) {      // (a model without geoms: one pass over none, every pixel a miss)
    const int ng = a.ngeom - g0 < GRX_CAM_STAGE ? a.ngeom - g0 : GRX_CAM_STAGE;
    const bool last = g0 + ng >= a.ngeom;
    __syncthreads();      // the previous pass has been traced and shaded
    if (t < ng) {
      grx_ray_stage(stage + t * GRX_RAY_REC, g0 + t, xpos, xquat, a.geom_type, a.geom_bodyid, a.geom_pos, a.geom_quat, a.geom_size, a.geom_rbound, a.plane_adr, a.plane_num);
      if (colors) for (int i = 0; i < 3; i++) cols[3 * t + i] = fminf(1.0f, fmaxf(colors[3 * (size_t)(g0 + t) + i], 0.0f));
    }
    __syncthreads();      // (thread 0's camera as well)
    float o[3], M[9];
    for (int i = 0; i < 3; i++) o[i] = cam[i];
    for (int i = 0; i < 9; i++) M[i] = cam[3 + i];
    const bool posed = cam[12] != 0.0f;
    if (t < ng) {
      const float* rec = stage + t * GRX_RAY_REC;
      const int* ri = (const int*)(rec + 16);
      int* q = rect + 4 * t;
      q[0] = 0; q[1] = W - 1; q[2] = 0; q[3] = H - 1;
      if (!posed || ri[1] == skip_a || ri[1] == skip_b || (ri[1] == 0 && !a.include_static)) { q[0] = 1; q[1] = 0; }
      else if (ri[0] != 0 && !(a.flags & GRX_CAM_NO_BINNING)) {
        const float w[3] = {rec[0] - o[0], rec[1] - o[1], rec[2] - o[2]};
        const float p[3] = {M[0] * w[0] + M[3] * w[1] + M[6] * w[2], M[1] * w[0] + M[4] * w[1] + M[7] * w[2], M[2] * w[0] + M[5] * w[1] + M[8] * w[2]};
        grx_cam_rect(p, rec[15] * 1.001f + 1e-6f, H, W, ax, ay, q);      // the radius grx_ray_geom rejects by
      }
    }
    __syncthreads();
    for (int c0 = 0; c0 < ntile; c0 += GRX_CAM_CHUNK) {
      const int nc = ntile - c0 < GRX_CAM_CHUNK ? ntile - c0 : GRX_CAM_CHUNK;
      if (t < nc) {
        const int ty = (c0 + t) / tiles_x, tx = (c0 + t) - ty * tiles_x;
        const int cl = tx * TW, ch = cl + TW - 1, rl = ty * TH, rh = rl + TH - 1;
        unsigned m[GRX_CAM_WORDS];
        for (int i = 0; i < GRX_CAM_WORDS; i++) m[i] = 0u;
        for (int g = 0; g < ng; g++) {
          const int4 q = *(const int4*)(rect + 4 * g);
          if (q.x <= ch && q.y >= cl && q.z <= rh && q.w >= rl && q.x <= q.y) m[g >> 5] |= 1u << (g & 31);
        }
        for (int i = 0; i < GRX_CAM_WORDS; i++) masks[i * GRX_CAM_CHUNK + t] = m[i];      // word-major: consecutive threads, consecutive banks
      }
      __syncthreads();
      for (int lt = wave; lt < nc; lt += GRX_CAM_BLOCK / 64) {
        const int ty = (c0 + lt) / tiles_x, tx = (c0 + lt) - ty * tiles_x;
        const int r = ty * TH + lane / TW, c = tx * TW + lane % TW;
        const bool live = r < H && c < W;
        const size_t at = image + (size_t)(live ? r : 0) * W + (live ? c : 0);
        const float u = grx_cam_u(c, W, ax), v = grx_cam_v(r, H, ay);
        const float d[3] = {M[0] * u + M[1] * v - M[2], M[3] * u + M[4] * v - M[5], M[6] * u + M[7] * v - M[8]};
        float best = -1.0f;
        int best_g = -1, won = -1;      // won: the staged index of a winner found in THIS pass
        if (g0 > 0 && live) {      // this lane's own store of the previous pass
          best = a.depth[at];
          if (a.seg) best_g = a.seg[at];
        }
        for (int i = 0; i < (ng + 31) / 32; i++) {
          unsigned m = __builtin_amdgcn_readfirstlane(masks[i * GRX_CAM_CHUNK + lt]);
          while (m) {
            const int g = 32 * i + __builtin_ctz(m);
            m &= m - 1u;
            if (live) {
              const float th = grx_ray_geom(stage + g * GRX_RAY_REC, o, d, a.planes);
              if (th >= 0.0f && (best < 0.0f || th < best)) { best = th; best_g = g0 + g; won = g; }
            }
          }
        }
        const float hit = best;      // the ray parameter the normal is taken at
        bool miss = false;
        if (live) {
          if (last) {
            grx_ray_finish(best, best_g, 1.0f, a.max_dist, &best, &best_g);
            miss = !(best >= 0.0f);
          }
          a.depth[at] = best;
          if (a.seg) a.seg[at] = best_g;
          if (miss) {
            if (s.rgba) s.rgba[at] = s.background;
            if (s.normal) for (int i = 0; i < 3; i++) s.normal[3 * at + i] = 0.0f;
          }
        }
        // SHADE: the wave's distinct winners, one at a time
        bool pending = live && !miss && won >= 0;
        while (pending) {
          const int g = __builtin_amdgcn_readfirstlane(won);      // the winner of the first unshaded lane: wave-uniform
          if (won == g) {
            const float* rec = stage + g * GRX_RAY_REC;
            float n[3];
            grx_shade_normal(rec, o, d, hit, a.planes, n);
            if (s.normal) for (int i = 0; i < 3; i++) s.normal[3 * at + i] = n[i];
            if (s.rgba) {
              const float sc = grx_shade_scale(n, d, s.light);
              s.rgba[at] = grx_shade_pack(cols[3 * g] * sc, cols[3 * g + 1] * sc, cols[3 * g + 2] * sc, 255u);
            }
            pending = false;
          }
        }
      }
      __syncthreads();      // the chunk's masks have been read
    }
  }
}

// waves_per_eu(5, 5): the depth kernel's five waves per SIMD.  Left alone the compiler takes 103 VGPRs, four waves, and the trace loop -- the same loop -- ran a quarter slower
// (profiles/camera_probe.txt); held to 96 it spills nothing to scratch.
extern "C" __global__ void __launch_bounds__(GRX_CAM_BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5)))
grx_camera_rgb_kernel(GrxCamRgbArgs s) {
  __shared__ float stage[GRX_CAM_STAGE * GRX_RAY_REC];
  __shared__ float cols[GRX_CAM_STAGE * 3];
  __shared__ __attribute__((aligned(16))) int rect[GRX_CAM_STAGE * 4];
  __shared__ unsigned masks[GRX_CAM_WORDS * GRX_CAM_CHUNK];
  __shared__ float cam[16];
  if (s.c.mask && !s.c.mask[blockIdx.x]) return;      // a masked-out world's images keep their bits (the whole workgroup leaves)
  if (s.c.flags & GRX_CAM_TILE_16X4) grx_camera_rgb_image<16, 4>(s, stage, cols, rect, masks, cam);
  else grx_camera_rgb_image<8, 8>(s, stage, cols, rect, masks, cam);
}

extern "C" int grx_tu_camera_rgb_launch(const GrxCamRgbArgs* s, void* stream) {
  hipLaunchKernelGGL(grx_camera_rgb_kernel, dim3((unsigned)s->c.n_worlds, (unsigned)s->c.n_cams), dim3(GRX_CAM_BLOCK), 0, (hipStream_t)stream, *s);
  return (int)hipGetLastError();
}
