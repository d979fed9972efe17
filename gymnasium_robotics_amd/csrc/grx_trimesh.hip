// grx_trimesh.hip -- the kernels behind mesh="triangles" (include/grx_capi.h grx_sim_ray_tri / grx_sim_ray_sites_tri / grx_sim_render_tri): the ray kernel and the depth /
// segmentation render kernel in the variant that sees a mesh geom's TRIANGLES through a bounding-volume hierarchy instead of its convex hull.  A translation unit of its own
// next to grx_rays.hip and grx_camera.hip, which stay what they are; the routines are csrc/grx_trimesh.h.
//
// RAYS.  grx_rays.hip's kernel with one call replaced: the same lane <-> ray map (grx_ray_shape), the same staging of geom records in LDS (grx_ray_stage -- with the
// hierarchy's per-geom table where the hull planes' was, so a mesh's record carries its first node and first triangle), the same filters and the same tie rule.  A geom that
// is no mesh goes through grx_ray_geom; a mesh passes its bounding sphere and then the lane walks the hierarchy on its own (grx_ray_trimesh: stackless, one integer of state),
// reading nodes and triangles from global memory.  Lanes of a workgroup's rays have unrelated origins, so there is nothing to share between them.
//
// CAMERAS ("Cameras").  grx_camera.hip's STAGE, BIN and TRACE: one workgroup of 256 threads per (world, camera) image, geoms binned to 8 x 8 pixel tiles by their
// bounding spheres, a wave per tile, a lane per pixel, the tile's set bits walked in ascending geom id.  What is new is what happens at a mesh bit:
//   WAVE WALK   the 64 lanes of a tile share an origin and span a small solid angle, so they walk a mesh's hierarchy TOGETHER: the node index is wave-uniform (a scalar
//               register), every lane tests the node's box against its own ray and its own best t, and a vote (__any) decides: no lane enters -- the whole wave takes the skip
//               link; some lane enters an inner node -- on to the first child; a leaf -- the lanes that entered test its triangles, each keeping its own best.  A lane's result
//               depends on its own ray only (it tests a triangle iff its own box test passed), so binning, tile shape and neighbours cannot change a pixel.
//   LDS WINDOW  a node is fetched once per wave: as an LDS broadcast from a window of GRX_TRI_WINDOW nodes (16 KiB) beside the geom stage, into which the workgroup copies, once
//               per image and staging pass, the hierarchies of the pass's visible meshes that fit (ascending geom id, geoms of one mesh share a copy); a mesh that does not fit
//               is read from global memory through the same wave-uniform index.  Triangles are always read from global memory.
// Multi-pass models and chunked images carry a pixel's best hit in the output image, as grx_camera.hip does.
#include <hip/hip_runtime.h>

#include "grx_camera.h"
#include "grx_trimesh.h"

#define GRX_TRI_WINDOW 512      // nodes of the LDS window
// LDS of a render workgroup: grx_camera.hip's 16436 B, the window 512 * 32 = 16384 B and two tables of 128 ints: 33844 B, four workgroups of a CU's 160 KiB

extern "C" __global__ void __launch_bounds__(GRX_RAY_BLOCK)
grx_trimesh_ray_kernel(GrxRayArgs a, GrxTriArgs m, int rpb, int wpb, int gtile, int stride) {
  __shared__ float stage[GRX_RAY_STAGE * GRX_RAY_REC];
  const int t = threadIdx.x, wl = t / rpb, rl = t - wl * rpb;
  const int w0 = blockIdx.x * wpb, world = w0 + wl, ray = blockIdx.y * rpb + rl;
  bool live = wl < wpb && world < a.n_worlds && ray < a.n_rays;
  if (live && a.mask && !a.mask[world]) live = false;      // a masked-out world's rows keep their bits
  float o[3] = {0.0f, 0.0f, 0.0f}, dn[3] = {0.0f, 0.0f, 1.0f}, scale = 1.0f;
  int skip_a = -1, skip_b = -1;
  bool cast = false;
  if (live) {
    float d[3];
    if (a.sites) {
      const int s = a.ray_site[ray];
      const float* sp = a.site_xpos + ((size_t)world * a.nsite + s) * 3;
      const float* sm = a.site_xmat + ((size_t)world * a.nsite + s) * 9;
      const float* l = a.local_dir + 3 * (size_t)ray;
      for (int k = 0; k < 3; k++) { o[k] = sp[k]; d[k] = sm[3 * k] * l[0] + sm[3 * k + 1] * l[1] + sm[3 * k + 2] * l[2]; }
      if (a.exclude_site_body) skip_b = a.site_bodyid[s];
    } else {
      const size_t at = ((size_t)world * a.n_rays + ray) * 3;
      for (int k = 0; k < 3; k++) { o[k] = a.origin[at + k]; d[k] = a.direction[at + k]; }
    }
    if (a.exclude_body) skip_a = a.exclude_body[ray];
    cast = grx_ray_prepare(o, d, dn, &scale);
  }
  float best = -1.0f;
  int best_g = -1;
  for (int g0 = 0; g0 < a.ngeom; g0 += gtile) {
    const int ng = a.ngeom - g0 < gtile ? a.ngeom - g0 : gtile;
    __syncthreads();      // the previous tile has been read
    for (int i = t; i < wpb * ng; i += blockDim.x) {
      const int sw = i / ng, sg = i - sw * ng;
      if (w0 + sw < a.n_worlds)
        grx_ray_stage(stage + (size_t)sw * stride + (size_t)sg * GRX_RAY_REC, g0 + sg, a.xpos + (size_t)(w0 + sw) * a.nbody * 3, a.xquat + (size_t)(w0 + sw) * a.nbody * 4, a.geom_type, a.geom_bodyid,
                      a.geom_pos, a.geom_quat, a.geom_size, a.geom_rbound, m.geom_adr, m.geom_adr + a.ngeom);
    }
    __syncthreads();
    if (cast) grx_tri_tile(stage + (size_t)wl * stride, ng, g0, o, dn, m.nodes, m.tris, skip_a, skip_b, a.include_static, &best, &best_g);
  }
  if (live) {
    float dist;
    grx_ray_finish(best, best_g, scale, a.max_dist, &dist, &best_g);
    const size_t at = (size_t)world * a.n_rays + ray;
    a.dist[at] = dist;
    if (a.geom) a.geom[at] = best_g;
  }
}

extern "C" int grx_tu_trimesh_rays_launch(const GrxRayArgs* a, const GrxTriArgs* m, void* stream) {
  const GrxRayShape s = grx_ray_shape(a->n_rays);
  const dim3 grid((unsigned)((a->n_worlds + s.wpb - 1) / s.wpb), (unsigned)((a->n_rays + s.rpb - 1) / s.rpb));
  hipLaunchKernelGGL(grx_trimesh_ray_kernel, grid, dim3((unsigned)s.threads), 0, (hipStream_t)stream, *a, *m, s.rpb, s.wpb, s.gtile, s.stride);
  return (int)hipGetLastError();
}

// THE WAVE WALK of one mesh: every lane of the wave calls it together (no lane may have left), `want` says whether this lane's ray is a candidate at all.  nodes: the mesh's
// first node, in the LDS window or in global memory; i, the skip link and the leaf word are wave-uniform and held in scalar registers.
__device__ __forceinline__ float grx_tri_wave(const int* nodes, const float* tris, const GrxTriRay& r, bool want, float best) {
  int i = 0;
  while (i >= 0) {
    const int* nd = nodes + (size_t)i * GRX_TRI_NODE;
    float box[6];
    for (int k = 0; k < 6; k++) box[k] = ((const float*)nd)[k];
    const int skip = __builtin_amdgcn_readfirstlane(nd[6]), leaf = __builtin_amdgcn_readfirstlane(nd[7]);
    const bool in = want && grx_tri_box(box, r, best);
    if (!__any(in)) { i = skip; continue; }
    if (leaf < 0) { i++; continue; }
    if (in) best = grx_tri_leaf(tris, leaf, r, best);
    i = skip;
  }
  return best;
}

template <int TW, int TH>
__device__ __forceinline__ void grx_trimesh_image(const GrxCamArgs& a, const GrxTriArgs& m, float* stage, int* rect, unsigned* masks, float* cam, int* window, int* win, int* wcopy) {
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
    if (t < ng) grx_ray_stage(stage + t * GRX_RAY_REC, g0 + t, xpos, xquat, a.geom_type, a.geom_bodyid, a.geom_pos, a.geom_quat, a.geom_size, a.geom_rbound, m.geom_adr, m.geom_adr + a.ngeom);
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
        grx_cam_rect(p, rec[15] * 1.001f + 1e-6f, H, W, ax, ay, q);      // the radius the bounding-sphere test rejects by
      }
    }
    __syncthreads();
    // WINDOW: thread 0 gives every visible mesh of the pass a place in the window while there is room (win: first node there, -1: read it from global memory; wcopy: the
    // nodes its first geom copies), then the workgroup copies
    if (t == 0) {
      int used = 0;
      for (int g = 0; g < ng; g++) {
        const int* ri = (const int*)(stage + g * GRX_RAY_REC + 16);
        win[g] = -1; wcopy[g] = 0;
        if (ri[0] != 7 || ri[2] < 0 || rect[4 * g] > rect[4 * g + 1] || (m.flags & (GRX_TRI_NO_WINDOW | GRX_TRI_PER_LANE))) continue;
        for (int h = 0; h < g && win[g] < 0; h++)
          if (win[h] >= 0 && ((const int*)(stage + h * GRX_RAY_REC + 16))[2] == ri[2]) win[g] = win[h];
        const int n = m.geom_adr[2 * a.ngeom + g0 + g];
        if (win[g] < 0 && n > 0 && used + n <= GRX_TRI_WINDOW) { win[g] = used; wcopy[g] = n; used += n; }
      }
    }
    __syncthreads();
    for (int g = 0; g < ng; g++) {
      const int n = wcopy[g] * GRX_TRI_NODE;
      if (n == 0) continue;
      const int* src = m.nodes + (size_t)((const int*)(stage + g * GRX_RAY_REC + 16))[2] * GRX_TRI_NODE;
      int* dst = window + win[g] * GRX_TRI_NODE;
      for (int i = t; i < n; i += GRX_CAM_BLOCK) dst[i] = src[i];
    }
    __syncthreads();
    for (int c0 = 0; c0 < ntile; c0 += GRX_CAM_CHUNK) {
      const int nc = ntile - c0 < GRX_CAM_CHUNK ? ntile - c0 : GRX_CAM_CHUNK;
      if (t < nc) {
        const int ty = (c0 + t) / tiles_x, tx = (c0 + t) - ty * tiles_x;
        const int cl = tx * TW, ch = cl + TW - 1, rl = ty * TH, rh = rl + TH - 1;
        unsigned mk[GRX_CAM_WORDS];
        for (int i = 0; i < GRX_CAM_WORDS; i++) mk[i] = 0u;
        for (int g = 0; g < ng; g++) {
          const int4 q = *(const int4*)(rect + 4 * g);
          if (q.x <= ch && q.y >= cl && q.z <= rh && q.w >= rl && q.x <= q.y) mk[g >> 5] |= 1u << (g & 31);
        }
        for (int i = 0; i < GRX_CAM_WORDS; i++) masks[i * GRX_CAM_CHUNK + t] = mk[i];      // word-major: consecutive threads, consecutive banks
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
          unsigned mk = __builtin_amdgcn_readfirstlane(masks[i * GRX_CAM_CHUNK + lt]);
          while (mk) {
            const int g = 32 * i + __builtin_ctz(mk);
            mk &= mk - 1u;
            const float* rec = stage + g * GRX_RAY_REC;
            const int* ri = (const int*)(rec + 16);
            const int type = __builtin_amdgcn_readfirstlane(ri[0]), first = __builtin_amdgcn_readfirstlane(ri[2]);
            float th = -1.0f;
            if (type != 7 || (m.flags & GRX_TRI_PER_LANE)) {      // wave-uniform
              if (live) th = grx_tri_geom(rec, o, d, m.nodes, m.tris, best);
            } else if (first >= 0) {      // every lane of the wave goes in: the walk votes
              const float w[3] = {o[0] - rec[0], o[1] - rec[1], o[2] - rec[2]};
              const bool want = live && grx_tri_sphere(w, d, rec[15]);
              if (__any(want)) {
                float p[3], dl[3];
                GrxTriRay ray;
                grx_tri_local(rec, o, d, p, dl);
                grx_tri_ray(p, dl, &ray);
                const float* tris = m.tris + (size_t)__builtin_amdgcn_readfirstlane(ri[3]) * GRX_TRI_WORDS;
                const int wn = __builtin_amdgcn_readfirstlane(win[g]);
                const float tm = wn >= 0 ? grx_tri_wave(window + wn * GRX_TRI_NODE, tris, ray, want, best) : grx_tri_wave(m.nodes + (size_t)first * GRX_TRI_NODE, tris, ray, want, best);
                if (want) th = tm;
              }
            }
            if (th >= 0.0f && (best < 0.0f || th < best)) { best = th; best_g = g0 + g; }
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
grx_trimesh_render_kernel(GrxCamArgs a, GrxTriArgs m) {
  __shared__ float stage[GRX_CAM_STAGE * GRX_RAY_REC];
  __shared__ __attribute__((aligned(16))) int rect[GRX_CAM_STAGE * 4];
  __shared__ unsigned masks[GRX_CAM_WORDS * GRX_CAM_CHUNK];
  __shared__ float cam[16];
  __shared__ int window[GRX_TRI_WINDOW * GRX_TRI_NODE];
  __shared__ int win[GRX_CAM_STAGE], wcopy[GRX_CAM_STAGE];
  if (a.mask && !a.mask[blockIdx.x]) return;      // a masked-out world's images keep their bits (the whole workgroup leaves)
  if (a.flags & GRX_CAM_TILE_16X4) grx_trimesh_image<16, 4>(a, m, stage, rect, masks, cam, window, win, wcopy);
  else grx_trimesh_image<8, 8>(a, m, stage, rect, masks, cam, window, win, wcopy);
}

extern "C" int grx_tu_trimesh_render_launch(const GrxCamArgs* a, const GrxTriArgs* m, void* stream) {
  hipLaunchKernelGGL(grx_trimesh_render_kernel, dim3((unsigned)a->n_worlds, (unsigned)a->n_cams), dim3(GRX_CAM_BLOCK), 0, (hipStream_t)stream, *a, *m);
  return (int)hipGetLastError();
}
