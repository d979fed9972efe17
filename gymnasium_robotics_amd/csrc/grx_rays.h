// grx_rays.h -- ray casting against the compiled model's geoms (include/grx_capi.h grx_sim_ray / grx_sim_ray_sites): the per-ray, per-geom routines, the staged geom
// record, the loop over one ray's geoms, and the host-side derivation of the hulls' face planes.  A header of its own, outside the engine template: csrc/grx_rays.hip compiles
// it for gfx950, tests/emu/grx_emu_rays.cpp for the host.  (grx_ray_sphere / _box / _cylinder of csrc/grx_eng_sensors.h are the touch zones' routines and stay what they are;
// the ones here are written for world-scale rays: they work from the ray's closest point to the centre, not from b*b - a*c, whose cancellation grows with the distance.)
//
// DEFINITION.  A ray is o + t d, t >= 0.  Every routine takes the ray in the geom's own frame (p, d) and returns the smallest t >= 0 at which it meets the geom's SURFACE, or
// -1: the entry point from outside, the exit point from inside.  d need not be unit (the callers pass it scaled to max |d_i| = 1 and rescale t).  A plane is one-sided.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GRX_RAY_FN __host__ __device__ static inline
#else
#define GRX_RAY_FN static inline
#endif

#define GRX_RAY_REC 20        // words of a staged geom record: pos 3, mat 9 (row-major, geom -> world), size 3, rbound, then type, body, first plane, planes as ints
#define GRX_RAY_STAGE 512     // records of the staging area (40 KiB of LDS): worlds of a workgroup x geoms of a tile
#define GRX_RAY_BLOCK 256     // largest workgroup

GRX_RAY_FN float grx_ray_min(float best, float t) { return (t >= 0.0f && (best < 0.0f || t < best)) ? t : best; }

// plane z = 0 with normal +z, half sizes sx, sy (<= 0: infinite in that direction)
GRX_RAY_FN float grx_ray_hit_plane(const float* p, const float* d, float sx, float sy) {
  if (!(d[2] < 0.0f)) return -1.0f;
  const float t = -p[2] / d[2];
  if (!(t >= 0.0f)) return -1.0f;
  if (sx > 0.0f && fabsf(p[0] + t * d[0]) > sx) return -1.0f;
  if (sy > 0.0f && fabsf(p[1] + t * d[1]) > sy) return -1.0f;
  return t;
}

// the two parameters at which p + t d is at distance r from the origin, over the first `dim` coordinates (3: a sphere, 2: the infinite cylinder about z); false: none
GRX_RAY_FN bool grx_ray_roots(const float* p, const float* d, int dim, float r, float* t0, float* t1) {
  float a = 0.0f, b = 0.0f;
  for (int k = 0; k < dim; k++) { a += d[k] * d[k]; b += d[k] * p[k]; }
  if (!(a > 1e-30f)) return false;
  const float tc = -b / a;      // the closest point q of the line: |p + t d|^2 = |q|^2 + (t - tc)^2 a
  float qq = 0.0f;
  for (int k = 0; k < dim; k++) { const float q = p[k] + tc * d[k]; qq += q * q; }
  const float h = (r * r - qq) / a;
  if (!(h >= 0.0f)) return false;
  const float s = sqrtf(h);
  *t0 = tc - s; *t1 = tc + s;
  return true;
}

GRX_RAY_FN float grx_ray_hit_sphere(const float* p, const float* d, float r) {
  float t0, t1;
  if (!grx_ray_roots(p, d, 3, r, &t0, &t1)) return -1.0f;
  return t0 >= 0.0f ? t0 : (t1 >= 0.0f ? t1 : -1.0f);
}

// ellipsoid with radii sz: scaled to the unit sphere, which leaves t as it is
GRX_RAY_FN float grx_ray_hit_ellipsoid(const float* p, const float* d, const float* sz) {
  const float ps[3] = {p[0] / sz[0], p[1] / sz[1], p[2] / sz[2]}, ds[3] = {d[0] / sz[0], d[1] / sz[1], d[2] / sz[2]};
  return grx_ray_hit_sphere(ps, ds, 1.0f);
}

// cylinder of radius r and half height h about z: the side between the caps, the caps inside the radius
GRX_RAY_FN float grx_ray_hit_cylinder(const float* p, const float* d, float r, float h) {
  float best = -1.0f, t0, t1;
  if (grx_ray_roots(p, d, 2, r, &t0, &t1)) {
    if (fabsf(p[2] + t0 * d[2]) <= h) best = grx_ray_min(best, t0);
    if (fabsf(p[2] + t1 * d[2]) <= h) best = grx_ray_min(best, t1);
  }
  if (d[2] != 0.0f)
    for (int side = -1; side <= 1; side += 2) {
      const float t = ((float)side * h - p[2]) / d[2], x = p[0] + t * d[0], y = p[1] + t * d[1];
      if (x * x + y * y <= r * r) best = grx_ray_min(best, t);
    }
  return best;
}

// capsule of radius r and half length h about z: the side between the end planes, and of each end sphere the half beyond its plane
GRX_RAY_FN float grx_ray_hit_capsule(const float* p, const float* d, float r, float h) {
  float best = -1.0f, t0, t1;
  if (grx_ray_roots(p, d, 2, r, &t0, &t1)) {
    if (fabsf(p[2] + t0 * d[2]) <= h) best = grx_ray_min(best, t0);
    if (fabsf(p[2] + t1 * d[2]) <= h) best = grx_ray_min(best, t1);
  }
  for (int side = -1; side <= 1; side += 2) {
    const float pe[3] = {p[0], p[1], p[2] - (float)side * h};
    if (!grx_ray_roots(pe, d, 3, r, &t0, &t1)) continue;
    if ((float)side * (pe[2] + t0 * d[2]) >= 0.0f) best = grx_ray_min(best, t0);
    if ((float)side * (pe[2] + t1 * d[2]) >= 0.0f) best = grx_ray_min(best, t1);
  }
  return best;
}

// a convex polytope as the half spaces n . x <= c (pl: n planes of (nx, ny, nz, c)): the ray is clipped against every plane; what is left is [enter, leave]
GRX_RAY_FN float grx_ray_hit_planes(const float* p, const float* d, const float* pl, int n) {
  float enter = -INFINITY, leave = INFINITY;
  for (int k = 0; k < n; k++) {
    const float* q = pl + 4 * k;
    const float nd = q[0] * d[0] + q[1] * d[1] + q[2] * d[2], gap = q[3] - (q[0] * p[0] + q[1] * p[1] + q[2] * p[2]);      // gap >= 0: p is on the inner side
    if (nd == 0.0f) { if (gap < 0.0f) return -1.0f; continue; }
    const float t = gap / nd;
    if (nd < 0.0f) enter = fmaxf(enter, t); else leave = fminf(leave, t);
  }
  if (!(enter <= leave) || !(leave >= 0.0f)) return -1.0f;
  const float t = enter >= 0.0f ? enter : leave;
  return (t >= 0.0f && t < INFINITY) ? t : -1.0f;
}

GRX_RAY_FN float grx_ray_hit_box(const float* p, const float* d, const float* sz) {
  const float pl[24] = {1, 0, 0, sz[0], -1, 0, 0, sz[0], 0, 1, 0, sz[1], 0, -1, 0, sz[1], 0, 0, 1, sz[2], 0, 0, -1, sz[2]};
  return grx_ray_hit_planes(p, d, pl, 6);
}

// A ray made safe: finite origin, finite non-zero direction scaled to max |d_i| = 1 (so no d . d underflows or overflows); *scale: t of the scaled ray = t of the caller's * scale
GRX_RAY_FN bool grx_ray_prepare(const float* o, const float* d, float* dn, float* scale) {
  const float s = fmaxf(fabsf(d[0]), fmaxf(fabsf(d[1]), fabsf(d[2])));
  if (!(s > 0.0f) || !(s < INFINITY) || !(d[0] == d[0]) || !(d[1] == d[1]) || !(d[2] == d[2])) return false;
  if (!(fabsf(o[0]) < INFINITY) || !(fabsf(o[1]) < INFINITY) || !(fabsf(o[2]) < INFINITY)) return false;
  dn[0] = d[0] / s; dn[1] = d[1] / s; dn[2] = d[2] / s; *scale = s;
  return true;
}

// one geom record (GRX_RAY_REC words) against the world-frame ray (o, dn); planes: the model's hull planes
GRX_RAY_FN float grx_ray_geom(const float* rec, const float* o, const float* dn, const float* planes) {
  const int* ri = (const int*)(rec + 16);
  const int type = ri[0];
  const float w[3] = {o[0] - rec[0], o[1] - rec[1], o[2] - rec[2]}, rb = rec[15];
  if (type != 0) {      // bounding sphere (planes have none): the ray starts outside it and points away, or passes it by
    const float a = dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2], b = dn[0] * w[0] + dn[1] * w[1] + dn[2] * w[2], rr = rb * 1.001f + 1e-6f;
    const float cc = w[0] * w[0] + w[1] * w[1] + w[2] * w[2] - rr * rr;
    if (cc > 0.0f) {
      if (b > 0.0f) return -1.0f;
      const float tc = -b / a, q[3] = {w[0] + tc * dn[0], w[1] + tc * dn[1], w[2] + tc * dn[2]};
      if (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] > rr * rr) return -1.0f;
    }
  }
  const float* R = rec + 3;
  const float p[3] = {R[0] * w[0] + R[3] * w[1] + R[6] * w[2], R[1] * w[0] + R[4] * w[1] + R[7] * w[2], R[2] * w[0] + R[5] * w[1] + R[8] * w[2]};
  const float d[3] = {R[0] * dn[0] + R[3] * dn[1] + R[6] * dn[2], R[1] * dn[0] + R[4] * dn[1] + R[7] * dn[2], R[2] * dn[0] + R[5] * dn[1] + R[8] * dn[2]};
  const float* sz = rec + 12;
  switch (type) {
    case 0: return grx_ray_hit_plane(p, d, sz[0], sz[1]);
    case 2: return grx_ray_hit_sphere(p, d, sz[0]);
    case 3: return grx_ray_hit_capsule(p, d, sz[0], sz[1]);
    case 4: return grx_ray_hit_ellipsoid(p, d, sz);
    case 5: return grx_ray_hit_cylinder(p, d, sz[0], sz[1]);
    case 6: return grx_ray_hit_box(p, d, sz);
    case 7: return ri[3] > 0 ? grx_ray_hit_planes(p, d, planes + 4 * (size_t)ri[2], ri[3]) : -1.0f;
    default: return -1.0f;
  }
}

// one ray against ng staged records (geoms g0 ...): ascending ids and a strict `<`, so the smaller id keeps a tie; skip_a / skip_b: excluded bodies (-1: none)
GRX_RAY_FN void grx_ray_tile(const float* recs, int ng, int g0, const float* o, const float* dn, const float* planes, int skip_a, int skip_b, int include_static, float* best, int* best_g) {
  for (int g = 0; g < ng; g++) {
    const float* rec = recs + g * GRX_RAY_REC;
    const int body = ((const int*)(rec + 16))[1];
    if (body == skip_a || body == skip_b || (body == 0 && !include_static)) continue;
    const float th = grx_ray_geom(rec, o, dn, planes);
    if (th >= 0.0f && (*best < 0.0f || th < *best)) { *best = th; *best_g = g0 + g; }
  }
}
// the ray's answer from the best hit of the scaled ray
GRX_RAY_FN void grx_ray_finish(float best, int best_g, float scale, float max_dist, float* dist, int* geom) {
  float t = best >= 0.0f ? best / scale : -1.0f;
  if (!(t >= 0.0f) || !(t < INFINITY) || (max_dist > 0.0f && t > max_dist)) { t = -1.0f; best_g = -1; }
  *dist = t; *geom = best_g;
}

// the record of geom g in a world whose bodies stand at xpos / xquat ([nbody, 3 / 4]): x_body o (geom_pos, geom_quat)
GRX_RAY_FN void grx_ray_stage(float* rec, int g, const float* xpos, const float* xquat, const int* geom_type, const int* geom_bodyid, const float* geom_pos, const float* geom_quat,
                              const float* geom_size, const float* geom_rbound, const int* plane_adr, const int* plane_num) {
  const int b = geom_bodyid[g];
  auto mat = [](const float* q, float* M) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    M[0] = w * w + x * x - y * y - z * z; M[1] = 2 * (x * y - w * z); M[2] = 2 * (x * z + w * y);
    M[3] = 2 * (x * y + w * z); M[4] = w * w - x * x + y * y - z * z; M[5] = 2 * (y * z - w * x);
    M[6] = 2 * (x * z - w * y); M[7] = 2 * (y * z + w * x); M[8] = w * w - x * x - y * y + z * z;
  };
  float B[9], G[9];
  mat(xquat + 4 * b, B); mat(geom_quat + 4 * g, G);
  const float* gp = geom_pos + 3 * g;
  for (int i = 0; i < 3; i++) {
    rec[i] = xpos[3 * b + i] + B[3 * i] * gp[0] + B[3 * i + 1] * gp[1] + B[3 * i + 2] * gp[2];
    for (int j = 0; j < 3; j++) rec[3 + 3 * i + j] = B[3 * i] * G[j] + B[3 * i + 1] * G[3 + j] + B[3 * i + 2] * G[6 + j];
  }
  rec[12] = geom_size[3 * g]; rec[13] = geom_size[3 * g + 1]; rec[14] = geom_size[3 * g + 2]; rec[15] = geom_rbound[g];
  int* ri = (int*)(rec + 16);
  ri[0] = geom_type[g]; ri[1] = b; ri[2] = plane_adr ? plane_adr[g] : 0; ri[3] = plane_num ? plane_num[g] : 0;
}

// HULL FACE PLANES, on the host, from the tables a model handle holds: vert [num, 3] and the adjacency of the hull's vertices (adjadr / adjnum per vertex, adj: neighbour ids
// local to the hull).  Every facet triangle of a convex hull is a triple of mutually adjacent vertices; such a triple is a face if every vertex lies on one side of its plane;
// triples of one (coplanar) face give one plane.  Appends (nx, ny, nz, c) with n . x <= c inside, n unit, to *out; returns the number of planes.
inline int grx_hull_planes(const double* vert, int num, const int32_t* adjadr, const int32_t* adjnum, const int32_t* adj, std::vector<float>* out) {
  std::vector<double> pl;
  double ext = 0.0;
  for (int k = 0; k < 3 * num; k++) ext = std::fmax(ext, std::fabs(vert[k]));
  // The vertices a handle holds are fp32: a vertex of a flat face lies up to a few 1e-7 of the hull's extent off the plane of three others, on either side, and the
  // adjacency triangulates such a face along diagonals chosen from the fp64 vertices.  So the side test allows that much (tol), a triple of a face folded the concave way is
  // still a face, the triples of one face merge within the same allowance (the widest triple's normal is kept), and every plane is pushed out to its support value
  // max_v n . v at the end: every vertex is inside every plane, and no face is lost to the choice of a diagonal.
  const double tol = 2e-6 * std::fmax(ext, 1e-3);
  std::vector<double> area;
  auto linked = [&](int a, int b) { for (int k = 0; k < adjnum[a]; k++) if (adj[adjadr[a] + k] == b) return true; return false; };
  for (int a = 0; a < num; a++)
    for (int ib = 0; ib < adjnum[a]; ib++) {
      const int b = adj[adjadr[a] + ib];
      if (b <= a || b >= num) continue;
      for (int ic = 0; ic < adjnum[a]; ic++) {
        const int c = adj[adjadr[a] + ic];
        if (c <= b || c >= num || !(linked(b, c) || linked(c, b))) continue;
        const double *A = vert + 3 * a, *Bv = vert + 3 * b, *C = vert + 3 * c;
        const double u[3] = {Bv[0] - A[0], Bv[1] - A[1], Bv[2] - A[2]}, v[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
        double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(len > 1e-8 * std::fmax(ext * ext, 1e-12))) continue;      // a degenerate triple
        n[0] /= len; n[1] /= len; n[2] /= len;
        double off = n[0] * A[0] + n[1] * A[1] + n[2] * A[2], lo = 0.0, hi = 0.0;
        for (int k = 0; k < num; k++) { const double s = n[0] * vert[3 * k] + n[1] * vert[3 * k + 1] + n[2] * vert[3 * k + 2] - off; lo = std::fmin(lo, s); hi = std::fmax(hi, s); }
        if (hi > tol && lo < -tol) continue;      // vertices on both sides: not a face
        if (hi > tol) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; off = -off; }
        bool dup = false;
        for (size_t k = 0; k < pl.size() && !dup; k += 4) {
          dup = std::fabs(pl[k] - n[0]) < 2e-5 && std::fabs(pl[k + 1] - n[1]) < 2e-5 && std::fabs(pl[k + 2] - n[2]) < 2e-5 && std::fabs(pl[k + 3] - off) < 4.0 * tol;
          if (dup && len > area[k / 4]) { pl[k] = n[0]; pl[k + 1] = n[1]; pl[k + 2] = n[2]; pl[k + 3] = off; area[k / 4] = len; }
        }
        if (!dup) { pl.push_back(n[0]); pl.push_back(n[1]); pl.push_back(n[2]); pl.push_back(off); area.push_back(len); }
      }
    }
  for (size_t k = 0; k < pl.size(); k += 4)
    for (int v = 0; v < num; v++) pl[k + 3] = std::fmax(pl[k + 3], pl[k] * vert[3 * v] + pl[k + 1] * vert[3 * v + 1] + pl[k + 2] * vert[3 * v + 2]);
  for (double x : pl) out->push_back((float)x);
  return (int)(pl.size() / 4);
}

// what a launch reads and writes: the model's tables on the device (the handle's), the planes derived above, and the caller's block (include/grx_capi.h grx_sim_rays)
struct GrxRayArgs {
  const int *geom_type, *geom_bodyid, *site_bodyid, *plane_adr, *plane_num;
  const float *geom_pos, *geom_quat, *geom_size, *geom_rbound, *planes;
  int ngeom, nbody, nsite;
  const float *xpos, *xquat, *origin, *direction, *site_xpos, *site_xmat, *local_dir;
  const int *ray_site, *exclude_body;      // ray_site: on the device here (the C ABI takes it from the host and keeps a device copy)
  const unsigned char* mask;
  float* dist; int* geom;
  float max_dist; int include_static, exclude_site_body, sites;      // sites != 0: the site-ray call
  int n_worlds, n_rays;
};

// The launch shape for R rays per world ("Rays"): a workgroup serves rpb consecutive rays of wpb consecutive worlds -- lane = world-in-group * rpb + ray-in-chunk --
// and stages gtile geoms of each of its worlds at a time, wpb * stride <= GRX_RAY_STAGE * GRX_RAY_REC words in all.
struct GrxRayShape { int rpb, wpb, threads, gtile, stride; };      // stride: words between two worlds' records in the staging area
inline GrxRayShape grx_ray_shape(int n_rays) {
  GrxRayShape s;
  s.rpb = n_rays < GRX_RAY_BLOCK ? n_rays : GRX_RAY_BLOCK;
  s.wpb = GRX_RAY_BLOCK / s.rpb; if (s.wpb > 64) s.wpb = 64; if (s.wpb < 1) s.wpb = 1;
  s.threads = ((s.wpb * s.rpb + 63) / 64) * 64;
  // worlds of one wave read the same word of their own records: an odd stride (one pad word per world) spreads them over the LDS banks, where gtile * GRX_RAY_REC words,
  // a multiple of 32 for every power-of-two wpb, would put all of them on one or two
  s.gtile = (GRX_RAY_STAGE * GRX_RAY_REC / s.wpb - (s.wpb > 1 ? 1 : 0)) / GRX_RAY_REC;
  s.stride = s.gtile * GRX_RAY_REC + (s.wpb > 1 ? 1 : 0);
  return s;
}
