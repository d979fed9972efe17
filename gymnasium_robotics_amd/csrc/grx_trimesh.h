// grx_trimesh.h -- rays against the TRIANGLES of a mesh geom (include/grx_capi.h grx_sim_ray_tri / grx_sim_ray_sites_tri / grx_sim_render_tri): the box and triangle tests, the
// stackless walk of a mesh's bounding-volume hierarchy, the geom routine that replaces a mesh's hull by its triangles, and the host-side check of a hierarchy.  A header of
// its own next to grx_rays.h, whose definition of a hit it keeps (the smallest t >= 0 on the SURFACE: entry from outside, exit from inside) and which it leaves untouched;
// host-compilable as that one is.  csrc/grx_trimesh.hip compiles it for gfx950.
//
// THE HIERARCHY (mjcf/compiler.py build_mesh_bvh makes it).  A node is GRX_TRI_NODE = 8 words: box min 3, box max 3 (fp32), then two ints: the SKIP LINK -- the node to visit
// when this node's box is missed or its subtree is done, always a later node or GRX_TRI_END -- and -1 for an inner node, first << 3 | count for a leaf.  The tree is flattened
// depth-first, so the first child of inner node i is node i + 1.  A walk is therefore one integer: hit an inner node, i + 1; anything else, the skip link.  No stack, so no
// per-lane array, no scratch memory and no LDS.  A triangle is GRX_TRI_WORDS = 9 floats, v0, e1 = v1 - v0, e2 = v2 - v0, in leaf order.  All indices are local to the mesh.
#pragma once
#include <string>

#include "grx_rays.h"

#define GRX_TRI_NODE 8
#define GRX_TRI_WORDS 9
#define GRX_TRI_END (-1)
#define GRX_TRI_LEAF 4          // most triangles of a leaf
#define GRX_TRI_MAX (1 << 20)   // most triangles of a mesh

// the ray in a mesh's frame, with the reciprocal direction the box test multiplies by
struct GrxTriRay { float p[3], d[3], inv[3]; };

// ZERO COMPONENTS.  inv[k] = 1 / d[k] is +-inf for d[k] = +-0, and (bound - p) * inf is -inf / +inf for an origin strictly between the two bounds (no constraint), the same
// infinity twice for one outside them (a miss): the ordering is right without a branch.  The one NaN, 0 * inf for an origin exactly ON a bound, is dropped by fminf / fmaxf,
// which return their other operand: the slab then reads as missed.  That is the right answer here, because every box of the hierarchy is strictly larger than what it holds
// (build_mesh_bvh), so a ray that runs inside a box's face plane meets none of the box's triangles.
GRX_RAY_FN void grx_tri_ray(const float* p, const float* d, GrxTriRay* r) {
  for (int k = 0; k < 3; k++) { r->p[k] = p[k]; r->d[k] = d[k]; r->inv[k] = 1.0f / d[k]; }
}

// RAY AGAINST BOX, the slab test: three multiply pairs.  True when the ray's [0, inf) meets the box no farther than `best` (best < 0: no bound).  The two comparisons allow
// 4 ulp: a slab parameter carries the rounding of one subtraction and one product, and a box must never be culled by that.
GRX_RAY_FN bool grx_tri_box(const float* box, const GrxTriRay& r, float best) {
  float tn = 0.0f, tf = INFINITY;
  for (int k = 0; k < 3; k++) {
    const float a = (box[k] - r.p[k]) * r.inv[k], b = (box[3 + k] - r.p[k]) * r.inv[k];
    tn = fmaxf(tn, fminf(a, b)); tf = fminf(tf, fmaxf(a, b));
  }
  return tn <= tf * 1.0000005f && (best < 0.0f || tn <= best * 1.0000005f);
}

// RAY AGAINST TRIANGLE, Moeller-Trumbore on (v0, e1, e2), two-sided: t >= 0 of the crossing, or -1.  A determinant of zero (a ray in the triangle's plane, a triangle without
// area) or one that is not finite is a miss.
GRX_RAY_FN float grx_tri_hit(const float* tr, const GrxTriRay& r) {
  const float *v0 = tr, *e1 = tr + 3, *e2 = tr + 6, *d = r.d;
  const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
  const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
  if (!(fabsf(det) > 0.0f) || !(fabsf(det) < INFINITY)) return -1.0f;
  const float inv = 1.0f / det, tv[3] = {r.p[0] - v0[0], r.p[1] - v0[1], r.p[2] - v0[2]};
  const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
  if (!(u >= 0.0f && u <= 1.0f)) return -1.0f;
  const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv;
  if (!(v >= 0.0f && u + v <= 1.0f)) return -1.0f;
  const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
  return (t >= 0.0f && t < INFINITY) ? t : -1.0f;
}

// the triangles of leaf word `leaf` against the ray: the smaller of best and their hits
GRX_RAY_FN float grx_tri_leaf(const float* tris, int leaf, const GrxTriRay& r, float best) {
  const float* tr = tris + (size_t)(leaf >> 3) * GRX_TRI_WORDS;
  for (int k = 0; k < (leaf & 7); k++) best = grx_ray_min(best, grx_tri_hit(tr + k * GRX_TRI_WORDS, r));
  return best;
}

// THE STACKLESS WALK of one mesh (nodes, tris: the mesh's first node and first triangle) by one ray in the mesh's frame: the smaller of `best` (< 0: none yet) and the
// smallest t >= 0 at which the ray meets a triangle.  A node whose box is missed, or lies farther than the running best, hands over to its skip link.
GRX_RAY_FN float grx_ray_trimesh(const int* nodes, const float* tris, const float* p, const float* d, float best) {
  GrxTriRay r;
  grx_tri_ray(p, d, &r);
  int i = 0;
  while (i >= 0) {
    const int* nd = nodes + (size_t)i * GRX_TRI_NODE;
    const int skip = nd[6], leaf = nd[7];
    if (!grx_tri_box((const float*)nd, r, best)) { i = skip; continue; }
    if (leaf < 0) { i++; continue; }
    best = grx_tri_leaf(tris, leaf, r, best);
    i = skip;
  }
  return best;
}

// the bounding-sphere rejection of grx_ray_geom, statement for statement (w = o - centre): false when the ray cannot meet the sphere of radius rb about the geom's centre
GRX_RAY_FN bool grx_tri_sphere(const float* w, const float* dn, float rb) {
  const float a = dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2], b = dn[0] * w[0] + dn[1] * w[1] + dn[2] * w[2], rr = rb * 1.001f + 1e-6f;
  const float cc = w[0] * w[0] + w[1] * w[1] + w[2] * w[2] - rr * rr;
  if (cc > 0.0f) {
    if (b > 0.0f) return false;
    const float tc = -b / a, q[3] = {w[0] + tc * dn[0], w[1] + tc * dn[1], w[2] + tc * dn[2]};
    if (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] > rr * rr) return false;
  }
  return true;
}
// the world-frame ray (o, dn) in the frame of the staged record rec
GRX_RAY_FN void grx_tri_local(const float* rec, const float* o, const float* dn, float* p, float* d) {
  const float w[3] = {o[0] - rec[0], o[1] - rec[1], o[2] - rec[2]}, *R = rec + 3;
  for (int k = 0; k < 3; k++) { p[k] = R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2]; d[k] = R[k] * dn[0] + R[3 + k] * dn[1] + R[6 + k] * dn[2]; }
}

// ONE GEOM RECORD against the world-frame ray, triangles for a mesh.  The record is grx_ray_stage's, staged with the hierarchy's per-geom table in place of the hull planes':
// its two last words are the mesh's first node and first triangle.  Everything but a mesh goes through grx_ray_geom unchanged.  Returns the geom's hit (-1: none); `best` only
// prunes the walk: a mesh farther than it may come back as a miss.
GRX_RAY_FN float grx_tri_geom(const float* rec, const float* o, const float* dn, const int* nodes, const float* tris, float best) {
  const int* ri = (const int*)(rec + 16);
  if (ri[0] != 7) return grx_ray_geom(rec, o, dn, nullptr);
  const float w[3] = {o[0] - rec[0], o[1] - rec[1], o[2] - rec[2]};
  if (ri[2] < 0 || !grx_tri_sphere(w, dn, rec[15])) return -1.0f;
  float p[3], d[3];
  grx_tri_local(rec, o, dn, p, d);
  const float t = grx_ray_trimesh(nodes + (size_t)ri[2] * GRX_TRI_NODE, tris + (size_t)ri[3] * GRX_TRI_WORDS, p, d, best);
  return (t >= 0.0f && (best < 0.0f || t < best)) ? t : -1.0f;
}

// grx_ray_tile with grx_tri_geom: one ray against ng staged records, ascending ids and a strict `<`
GRX_RAY_FN void grx_tri_tile(const float* recs, int ng, int g0, const float* o, const float* dn, const int* nodes, const float* tris, int skip_a, int skip_b, int include_static, float* best, int* best_g) {
  for (int g = 0; g < ng; g++) {
    const float* rec = recs + g * GRX_RAY_REC;
    const int body = ((const int*)(rec + 16))[1];
    if (body == skip_a || body == skip_b || (body == 0 && !include_static)) continue;
    const float th = grx_tri_geom(rec, o, dn, nodes, tris, *best);
    if (th >= 0.0f && (*best < 0.0f || th < *best)) { *best = th; *best_g = g0 + g; }
  }
}

// THE HOST'S CHECK of a hierarchy before it is uploaded: after it no walk can leave the arrays or fail to end.  nodes [n_nodes, 8], n_tris triangles, geom_adr [n_geom, 2] =
// (first node, first triangle) per geom, -1 / -1 for a geom without a mesh.  A mesh's nodes run from its first node to the next mesh's (or the end), its triangles likewise.
// count [n_geom] receives each geom's number of nodes (0: no mesh).  Returns "" or the reason.
inline std::string grx_tri_check(const int32_t* nodes, int n_nodes, int n_tris, const int32_t* geom_adr, int n_geom, std::vector<int32_t>* count) {
  count->assign((size_t)(n_geom > 0 ? n_geom : 0), 0);
  for (int g = 0; g < n_geom; g++) {
    const int na = geom_adr[2 * g], ta = geom_adr[2 * g + 1];
    if (na == -1 && ta == -1) continue;
    if (na < 0 || na >= n_nodes || ta < 0 || ta >= n_tris) return "geom " + std::to_string(g) + ": address (" + std::to_string(na) + ", " + std::to_string(ta) + ") is outside the node or the triangle array";
    int nn = n_nodes - na, nt = n_tris - ta;
    for (int h = 0; h < n_geom; h++) {
      if (geom_adr[2 * h] > na && geom_adr[2 * h] - na < nn) nn = geom_adr[2 * h] - na;
      if (geom_adr[2 * h + 1] > ta && geom_adr[2 * h + 1] - ta < nt) nt = geom_adr[2 * h + 1] - ta;
    }
    if (nt > GRX_TRI_MAX) return "geom " + std::to_string(g) + ": its mesh holds " + std::to_string(nt) + " triangles, more than " + std::to_string(GRX_TRI_MAX);
    (*count)[g] = nn;
    bool seen = false;
    for (int h = 0; h < g && !seen; h++) seen = geom_adr[2 * h] == na && geom_adr[2 * h + 1] == ta;
    if (seen) continue;      // a mesh two geoms share is checked once
    for (int i = 0; i < nn; i++) {
      const int32_t* nd = nodes + (size_t)(na + i) * GRX_TRI_NODE;
      const std::string at = "geom " + std::to_string(g) + ", node " + std::to_string(i) + ": ";
      if (nd[6] != GRX_TRI_END && (nd[6] <= i || nd[6] >= nn)) return at + "skip link " + std::to_string(nd[6]) + " is not a later node of the mesh's " + std::to_string(nn) + " (a backward link would never end)";
      if (nd[7] < 0) {
        if (i + 1 >= nn) return at + "an inner node without a first child";
        continue;
      }
      const int first = nd[7] >> 3, num = nd[7] & 7;
      if (num < 1 || num > GRX_TRI_LEAF) return at + "a leaf of " + std::to_string(num) + " triangles (1 .. " + std::to_string(GRX_TRI_LEAF) + ")";
      if (first + num > nt) return at + "leaf range " + std::to_string(first) + " + " + std::to_string(num) + " is past the end of the mesh's " + std::to_string(nt) + " triangles";
    }
  }
  return "";
}

// what the two kernels of csrc/grx_trimesh.hip read of a hierarchy, on the device: an argument block of its own next to GrxRayArgs / GrxCamArgs, which stay what they are
struct GrxTriArgs {
  const int* nodes;        // [M, 8]
  const float* tris;       // [T, 9]
  const int* geom_adr;     // [3, ngeom]: first node, first triangle (-1: no mesh), number of nodes
  int flags;
};
#define GRX_TRI_PER_LANE 1      // flags: the render kernel walks a mesh lane by lane (grx_ray_trimesh) instead of as a wave (A/B runs)
#define GRX_TRI_NO_WINDOW 2     // flags: the render kernel reads every node from global memory (A/B runs)
