// grx_camera.hip -- the render kernel of the task-free stepper's depth / segmentation cameras (include/grx_capi.h grx_sim_render), a translation unit of its own next to
// grx_rays.hip: it shares the hit routines and the staged geom record of csrc/grx_rays.h with the ray kernel and nothing with the step kernels.
//
// SHAPE ("Cameras").  One workgroup of 256 threads serves one (world, camera) image.  A camera's rays share an origin and form a regular fan, so the geoms are
// binned to screen tiles once per image and a tile tests only what may touch it:
//   STAGE  the workgroup builds the world-frame records of up to GRX_CAM_STAGE geoms of its world in LDS (grx_ray_stage), and thread 0 the camera's pose -- from the body
//          poses and the per-camera tables of the argument block, or from the caller's pose rows -- which every lane then reads as an LDS broadcast;
//   BIN    thread g moves geom g's bounding sphere to the camera frame and writes its pixel rectangle (grx_cam_rect; a plane: every pixel; a filtered geom: none); then thread t
//          builds the bit mask of tile t in registers from the rectangles (LDS broadcasts, no atomics: deterministic) and writes its GRX_CAM_WORDS words to LDS;
//   TRACE  a wave takes one tile at a time, lane <-> pixel (8 x 8: lane = 8 * row + column; or, by a flag, 16 x 4, whose four 64-byte row segments per store did not pay for its wider tiles), reads the tile's mask
//          words (wave-uniform, held in scalar registers) and walks the set bits in ascending geom id, every lane calling grx_ray_geom for its pixel: the type switch stays
//          wave-uniform, and ascending ids with a strict `<` keep the smaller-id tie rule of the ray kernel.
// Models with more geoms than one pass stages are walked in passes; a pixel's best hit is carried from pass to pass in the output image itself: the lane that wrote a pixel is
// the lane that reads it back (the tile -> wave -> lane map does not depend on the pass), so no other thread's store is ever read.  Images with more than GRX_CAM_CHUNK tiles
// are binned and traced a chunk of tiles at a time.  Pixels beyond the image's edge in an edge tile are masked lanes.
#include <hip/hip_runtime.h>

#include "grx_camera.h"

template <int TW, int TH>
__device__ __forceinline__ void grx_camera_image(const GrxCamArgs& a, float* stage, int* rect, unsigned* masks, float* cam) {
  static_assert(TW * TH == 64, "a tile is a wave");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int world = blockIdx.x, k = blockIdx.y, H = a.height, W = a.width;
  const float* xpos = a.xpos + (size_t)world * a.nbody * 3;
  const float* xquat = a.xquat + (size_t)world * a.nbody * 4;
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
    __syncthreads();      // the previous pass has been traced
    if (t < ng) grx_ray_stage(stage + t * GRX_RAY_REC, g0 + t, xpos, xquat, a.geom_type, a.geom_bodyid, a.geom_pos, a.geom_quat, a.geom_size, a.geom_rbound, a.plane_adr, a.plane_num);
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
        int best_g = -1;
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
              if (th >= 0.0f && (best < 0.0f || th < best)) { best = th; best_g = g0 + g; }
            }
          }
        }
        if (live) {
          if (last) grx_ray_finish(best, best_g, 1.0f, a.max_dist, &best, &best_g);
          a.depth[at] = best;
          if (a.seg) a.seg[at] = best_g;
        }
      }
      __syncthreads();      // the chunk's masks have been read
    }
  }
}

extern "C" __global__ void __launch_bounds__(GRX_CAM_BLOCK)
grx_camera_kernel(GrxCamArgs a) {
  __shared__ float stage[GRX_CAM_STAGE * GRX_RAY_REC];
  __shared__ __attribute__((aligned(16))) int rect[GRX_CAM_STAGE * 4];
  __shared__ unsigned masks[GRX_CAM_WORDS * GRX_CAM_CHUNK];
  __shared__ float cam[16];
  if (a.mask && !a.mask[blockIdx.x]) return;      // a masked-out world's images keep their bits (the whole workgroup leaves)
  if (a.flags & GRX_CAM_TILE_16X4) grx_camera_image<16, 4>(a, stage, rect, masks, cam);
  else grx_camera_image<8, 8>(a, stage, rect, masks, cam);
}

extern "C" int grx_tu_camera_launch(const GrxCamArgs* a, void* stream) {
  hipLaunchKernelGGL(grx_camera_kernel, dim3((unsigned)a->n_worlds, (unsigned)a->n_cams), dim3(GRX_CAM_BLOCK), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
