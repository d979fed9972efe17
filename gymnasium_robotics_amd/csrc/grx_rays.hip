// grx_rays.hip -- the ray-casting kernel of the task-free stepper (include/grx_capi.h grx_sim_ray / grx_sim_ray_sites), a translation unit of its own: it shares no code with the
// step kernels and is linked into libgrx_hip.so next to the units of grx_kernels.hip, whose C ABI checks the arguments and calls grx_tu_rays_launch.
//
// SHAPE ("Rays").  A workgroup serves rpb consecutive rays of wpb consecutive worlds (grx_ray_shape): thread = world-in-group * rpb + ray-in-chunk.  R >= 256: one world
// and 256 rays per workgroup; R = 64: four worlds; R = 1 (a rangefinder): 64 worlds in one wave, so a ray costs a lane and not a wave.  The geoms are walked in tiles: the
// workgroup stages the world frames of gtile (about 512 / wpb) geoms of each of its worlds in LDS (GRX_RAY_REC words each, 40 KiB in all: four workgroups per CU), once per
// workgroup and not once per ray, then every thread walks the tile.  A world's records start `stride` words after the previous world's, an odd number: lanes of different
// worlds read the same word of their own records, and an odd stride puts them on different LDS banks.  All lanes test geom g in the same iteration and the model is the same in every world, so the type switch is
// wave-uniform; what diverges is the bounding-sphere rejection and the filters.  Ascending geom ids and a strict `<` make the smaller id win a tie.
#include <hip/hip_runtime.h>

#include "grx_rays.h"

extern "C" __global__ void __launch_bounds__(GRX_RAY_BLOCK)
grx_ray_kernel(GrxRayArgs a, int rpb, int wpb, int gtile, int stride) {
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
                      a.geom_pos, a.geom_quat, a.geom_size, a.geom_rbound, a.plane_adr, a.plane_num);
    }
    __syncthreads();
    if (cast) grx_ray_tile(stage + (size_t)wl * stride, ng, g0, o, dn, a.planes, skip_a, skip_b, a.include_static, &best, &best_g);
  }
  if (live) {
    float dist;
    grx_ray_finish(best, best_g, scale, a.max_dist, &dist, &best_g);
    const size_t at = (size_t)world * a.n_rays + ray;
    a.dist[at] = dist;
    if (a.geom) a.geom[at] = best_g;
  }
}

extern "C" int grx_tu_rays_launch(const GrxRayArgs* a, void* stream) {
  const GrxRayShape s = grx_ray_shape(a->n_rays);
  const dim3 grid((unsigned)((a->n_worlds + s.wpb - 1) / s.wpb), (unsigned)((a->n_rays + s.rpb - 1) / s.rpb));
  hipLaunchKernelGGL(grx_ray_kernel, grid, dim3((unsigned)s.threads), 0, (hipStream_t)stream, *a, s.rpb, s.wpb, s.gtile, s.stride);
  return (int)hipGetLastError();
}
