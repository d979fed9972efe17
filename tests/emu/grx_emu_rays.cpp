// grx_emu_rays.cpp -- csrc/grx_rays.h compiled for the host (tests/emu/emu_rays.py): the per-ray routines the ray kernel runs, one world and one ray at a time, and the
// derivation of the hull face planes.  TEST INFRASTRUCTURE ONLY.  The loop below is the kernel's (csrc/grx_rays.hip) without its lanes: stage a tile of records, walk it.
#include <cstring>
#include <vector>

#include "../../gymnasium_robotics_amd/csrc/grx_rays.h"

extern "C" {

// face planes of one hull: vert [num, 3] fp64, the adjacency of its vertices; planes [cap, 4] is written when it holds them all; returns the number of planes
int emu_hull_planes(const double* vert, int num, const int32_t* adjadr, const int32_t* adjnum, const int32_t* adj, float* planes, int cap) {
  std::vector<float> out;
  const int n = grx_hull_planes(vert, num, adjadr, adjnum, adj, &out);
  if (planes && n <= cap) memcpy(planes, out.data(), sizeof(float) * out.size());
  return n;
}

float emu_hit_planes(const float* p, const float* d, const float* planes, int n) { return grx_ray_hit_planes(p, d, planes, n); }

// n_rays rays against one world; gtile: geoms staged at a time (any value >= 1 gives the same answer: the tile test)
void emu_ray_cast(int ngeom, const int* geom_type, const int* geom_bodyid, const float* geom_pos, const float* geom_quat, const float* geom_size, const float* geom_rbound,
                  const int* plane_adr, const int* plane_num, const float* planes, const float* xpos, const float* xquat, int n_rays, const float* origin, const float* direction,
                  const int* exclude_body, int include_static, float max_dist, int gtile, float* dist, int* geom) {
  std::vector<float> stage((size_t)gtile * GRX_RAY_REC);
  for (int r = 0; r < n_rays; r++) {
    float dn[3], scale = 1.0f, best = -1.0f;
    int best_g = -1;
    const float* o = origin + 3 * r;
    const bool cast = grx_ray_prepare(o, direction + 3 * r, dn, &scale);
    for (int g0 = 0; g0 < ngeom && cast; g0 += gtile) {
      const int ng = ngeom - g0 < gtile ? ngeom - g0 : gtile;
      for (int g = 0; g < ng; g++)
        grx_ray_stage(stage.data() + (size_t)g * GRX_RAY_REC, g0 + g, xpos, xquat, geom_type, geom_bodyid, geom_pos, geom_quat, geom_size, geom_rbound, plane_adr, plane_num);
      grx_ray_tile(stage.data(), ng, g0, o, dn, planes, exclude_body ? exclude_body[r] : -1, -1, include_static, &best, &best_g);
    }
    grx_ray_finish(best, best_g, scale, max_dist, dist + r, geom + r);
  }
}

// the launch shape of R rays per world: out = (rpb, wpb, threads, gtile, stride)
void emu_ray_shape(int n_rays, int* out) {
  const GrxRayShape s = grx_ray_shape(n_rays);
  out[0] = s.rpb; out[1] = s.wpb; out[2] = s.threads; out[3] = s.gtile; out[4] = s.stride;
}
}
