// grx_shade.h -- what the colour / surface-normal cameras (include/grx_capi.h grx_sim_render_rgb) add to the hit routines of csrc/grx_rays.h: the outward normal of a geom's
// surface at a hit, and the shading rule that turns it into a packed RGBA8 pixel.  A header of its own, host-compilable as grx_rays.h is: csrc/grx_camera_rgb.hip compiles it
// for gfx950.
//
// THE NORMAL.  x = p + t d is the hit in the geom's own frame.  The result is the OUTWARD unit normal of the surface at x, also when the ray came from inside.  A surface made
// of faces answers with the face whose surface x lies NEAREST (x is on it up to rounding), the smaller index on a tie: a cylinder's caps (index 0) before its side, a box's
// faces in the order x, y, z, a hull's planes in the order of the model's plane table.
//
// THE COLOUR.  In fp32, in this order: v = -d / |d|;  s = ambient + diffuse |n . v|;  with a sun of unit direction u (the way the light travels):
// s += sun_diffuse max(0, n_f . (-u)), n_f = n flipped to face the viewer;  each channel = floor(255 min(1, c s) + 0.5), c the geom's colour clamped to [0, 1].
// No shadows, no specular term, no transparency: a self-contained shading model, not MuJoCo's OpenGL renderer.
#pragma once
#include "grx_camera.h"

// a / |a| into n; a zero (or non-finite) vector: +z
GRX_RAY_FN void grx_shade_unit(float ax, float ay, float az, float* n) {
  const float l = sqrtf(ax * ax + ay * ay + az * az);
  if (l > 0.0f && l < INFINITY) { n[0] = ax / l; n[1] = ay / l; n[2] = az / l; }
  else { n[0] = 0.0f; n[1] = 0.0f; n[2] = 1.0f; }
}

// the normal in the geom's frame; sz: the geom's sizes, pl / np: its hull planes (type 7)
GRX_RAY_FN void grx_shade_normal_local(int type, const float* sz, const float* pl, int np, const float* x, float* n) {
  n[0] = 0.0f; n[1] = 0.0f; n[2] = 1.0f;      // a plane, and whatever has no surface
  switch (type) {
    case 2: grx_shade_unit(x[0], x[1], x[2], n); break;
    case 3: grx_shade_unit(x[0], x[1], x[2] - fminf(fmaxf(x[2], -sz[1]), sz[1]), n); break;      // from the nearest point of the segment |z| <= h
    case 4: grx_shade_unit(x[0] / (sz[0] * sz[0]), x[1] / (sz[1] * sz[1]), x[2] / (sz[2] * sz[2]), n); break;
    case 5: {
      const float cap = fabsf(fabsf(x[2]) - sz[1]), side = fabsf(sqrtf(x[0] * x[0] + x[1] * x[1]) - sz[0]);
      if (cap <= side) n[2] = x[2] < 0.0f ? -1.0f : 1.0f;
      else grx_shade_unit(x[0], x[1], 0.0f, n);
      break;
    }
    case 6: {
      int face = 0;
      float gap = fabsf(fabsf(x[0]) - sz[0]);
      for (int i = 1; i < 3; i++) { const float e = fabsf(fabsf(x[i]) - sz[i]); if (e < gap) { gap = e; face = i; } }
      for (int i = 0; i < 3; i++) n[i] = i == face ? (x[i] < 0.0f ? -1.0f : 1.0f) : 0.0f;
      break;
    }
    case 7: {
      float gap = INFINITY;
      for (int k = 0; k < np; k++) {
        const float* q = pl + 4 * k;
        const float e = fabsf(q[0] * x[0] + q[1] * x[1] + q[2] * x[2] - q[3]);
        if (e < gap) { gap = e; n[0] = q[0]; n[1] = q[1]; n[2] = q[2]; }
      }
      break;
    }
    default: break;
  }
}

// the world-frame normal at parameter t of the world-frame ray (o, d) on the staged record rec (GRX_RAY_REC words); planes: the model's hull planes
GRX_RAY_FN void grx_shade_normal(const float* rec, const float* o, const float* d, float t, const float* planes, float* n) {
  const int* ri = (const int*)(rec + 16);
  const float* R = rec + 3;
  const float w[3] = {(o[0] - rec[0]) + t * d[0], (o[1] - rec[1]) + t * d[1], (o[2] - rec[2]) + t * d[2]};
  const float x[3] = {R[0] * w[0] + R[3] * w[1] + R[6] * w[2], R[1] * w[0] + R[4] * w[1] + R[7] * w[2], R[2] * w[0] + R[5] * w[1] + R[8] * w[2]};
  float l[3];
  grx_shade_normal_local(ri[0], rec + 12, ri[0] == 7 ? planes + 4 * (size_t)ri[2] : nullptr, ri[0] == 7 ? ri[3] : 0, x, l);
  for (int i = 0; i < 3; i++) n[i] = R[3 * i] * l[0] + R[3 * i + 1] * l[1] + R[3 * i + 2] * l[2];
}

// the light terms of a launch; sun: unit, read only when has_sun
struct GrxShadeLight { float ambient, diffuse, sun[3], sun_diffuse; int has_sun; };

// the scale s of the colour rule for the unit normal n seen along the ray direction d
GRX_RAY_FN float grx_shade_scale(const float* n, const float* d, const GrxShadeLight& L) {
  const float dl = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const float nv = -(n[0] * d[0] + n[1] * d[1] + n[2] * d[2]) / dl;
  float s = L.ambient + L.diffuse * fabsf(nv);
  if (L.has_sun) {
    const float ns = -(n[0] * L.sun[0] + n[1] * L.sun[1] + n[2] * L.sun[2]);
    s += L.sun_diffuse * fmaxf(0.0f, nv < 0.0f ? -ns : ns);
  }
  return s;
}

GRX_RAY_FN unsigned grx_shade_level(float x) { return (unsigned)floorf(255.0f * fminf(1.0f, fmaxf(x, 0.0f)) + 0.5f); }
// bytes R, G, B, A in memory order (little endian): one dword per pixel
GRX_RAY_FN unsigned grx_shade_pack(float r, float g, float b, unsigned alpha) { return grx_shade_level(r) | (grx_shade_level(g) << 8) | (grx_shade_level(b) << 16) | (alpha << 24); }

// what a launch of the shading kernel reads and writes: the depth kernel's block as it is, and the shade block of include/grx_capi.h (grx_sim_shade) with the sun made unit
struct GrxCamRgbArgs {
  GrxCamArgs c;
  unsigned* rgba;            // [N, K, H, W] packed RGBA8, or NULL
  float* normal;             // [N, K, H, W, 3], or NULL
  const float* colors;       // [ngeom, 3], or [N, ngeom, 3] with colors_per_world
  int colors_per_world;
  GrxShadeLight light;
  unsigned background;       // the packed pixel of a miss (alpha 0)
};
// LDS of a workgroup: the depth kernel's 16436 B and the staged colours, 128 * 3 * 4 = 1536 B: 17972 B.  It does not bound the occupancy: the kernel's registers do, at five
// waves per SIMD (five workgroups of 256 threads per CU), as for the depth kernel
