// grx_camera.h -- depth and segmentation cameras of the task-free stepper (include/grx_capi.h grx_sim_render): the launch's argument block, the pixel fan and the binning
// rule.  The hits are those of csrc/grx_rays.h (grx_ray_stage, grx_ray_geom), unchanged: a pixel's hit is a ray's hit.  csrc/grx_camera.hip compiles it for gfx950.
//
// CONVENTIONS (MuJoCo's).  The camera looks along -z of its frame, +x right, +y up; row 0 is the top row.  The centre of pixel (r, c) of an H x W image has the camera-frame
// direction ((2 (c + .5) / W - 1) tan(fovy / 2) W / H, (1 - 2 (r + .5) / H) tan(fovy / 2), -1): its z component is -1, so the ray parameter of a hit IS the planar depth (metres
// along the optical axis), which is what the depth image holds; the Euclidean range is depth * |direction|.
#pragma once
#include "grx_rays.h"

#define GRX_CAM_MAX 16          // cameras of one launch: their tables travel inside the launch's argument block
#define GRX_CAM_MAX_SIDE 1024   // largest height / width
#define GRX_CAM_BLOCK 256       // threads of a workgroup: one workgroup per (world, camera) image
#define GRX_CAM_STAGE 128       // geom records of one staging pass: 32 bits x GRX_CAM_WORDS mask words per tile
#define GRX_CAM_WORDS (GRX_CAM_STAGE / 32)
#define GRX_CAM_CHUNK GRX_CAM_BLOCK   // tiles binned at a time: thread t builds the mask of tile t of the chunk
// LDS of a workgroup: records 128 * 20 * 4 = 10240 B, rectangles 128 * 16 = 2048 B, masks 256 * 4 * 4 = 4096 B, the camera 52 B: 16436 B, nine workgroups of a CU's 160 KiB

#define GRX_CAM_NO_BINNING 1    // flags: every tile gets every geom (A/B runs, the identity test)
#define GRX_CAM_TILE_16X4 2     // flags: 16 x 4 pixel tiles instead of 8 x 8 (8 x 8 measured faster: profiles/camera_probe.txt)

struct GrxCamArgs {
  const int *geom_type, *geom_bodyid, *plane_adr, *plane_num;
  const float *geom_pos, *geom_quat, *geom_size, *geom_rbound, *planes;
  int ngeom, nbody;
  const float *xpos, *xquat;
  const float *pose_pos, *pose_mat;      // device [N, K, 3] / [N, K, 9] (camera -> world, row-major), or NULL: the per-camera tables below
  int cam_body[GRX_CAM_MAX];             // the body a camera rides on (also with pose_pos: -1)
  float cam_pos[GRX_CAM_MAX][3], cam_quat[GRX_CAM_MAX][4];      // in that body's frame
  float cam_tan[GRX_CAM_MAX];            // tan(fovy / 2)
  int exclude_body[GRX_CAM_MAX];         // -1: none
  const unsigned char* mask;
  float* depth; int* seg;
  float max_dist; int include_static, exclude_own_body, flags;
  int n_worlds, n_cams, height, width;
};

// the camera-frame x and y of pixel centre (r, c) at depth 1; ax = tan(fovy / 2) W / H, ay = tan(fovy / 2)
GRX_RAY_FN float grx_cam_u(int c, int width, float ax) { return (2.0f * ((float)c + 0.5f) / (float)width - 1.0f) * ax; }
GRX_RAY_FN float grx_cam_v(int r, int height, float ay) { return (1.0f - 2.0f * ((float)r + 0.5f) / (float)height) * ay; }

// THE BINNING RULE.  A geom's bounding sphere (centre p in the camera frame, radius rr) against the H x W pixel grid: rect = (c_lo, c_hi, r_lo, r_hi), inclusive, of the pixels
// whose centre ray may meet the sphere; c_lo > c_hi: none.  With z = -p[2] the depth of the centre: z + rr < 0, wholly behind the image plane, none (a hit has depth >= 0);
// z - rr <= 2 % of rr, the camera inside the sphere or within its radius of the centre's plane, every pixel; otherwise the sphere lies in front and x / depth over its points
// spans exactly the two tangents from the origin to the circle of radius rr about (p[0], z), (p[0] z -+ rr sqrt(p[0]^2 + z^2 - rr^2)) / (z^2 - rr^2), and y / depth likewise.
// The bounds are widened by 1e-4 (1 + |bound|) and by one pixel on each side: fp32 rounding of the projection moves a bound by far less.
GRX_RAY_FN void grx_cam_rect(const float* p, float rr, int height, int width, float ax, float ay, int* rect) {
  const float z = -p[2];
  rect[0] = 0; rect[1] = width - 1; rect[2] = 0; rect[3] = height - 1;
  if (z + rr < 0.0f) { rect[0] = 1; rect[1] = 0; return; }
  if (!(z - rr > 0.02f * rr)) return;      // (a NaN lands here: every pixel)
  const float den = z * z - rr * rr;
  float lo[2], hi[2];
  for (int k = 0; k < 2; k++) {
    const float s = rr * sqrtf(fmaxf(p[k] * p[k] + den, 0.0f)), m = p[k] * z;
    lo[k] = (m - s) / den; hi[k] = (m + s) / den;
    lo[k] -= 1e-4f * (1.0f + fabsf(lo[k])); hi[k] += 1e-4f * (1.0f + fabsf(hi[k]));
  }
  // column of u: (u / ax + 1) W / 2 - .5; row of v: (1 - v / ay) H / 2 - .5 (v up, rows down).  Clamped as floats, so nothing overflows an int; fmaxf / fminf turn a NaN into the wide bound
  const float hw = 0.5f * (float)width, hh = 0.5f * (float)height;
  const float c_lo = ceilf((lo[0] / ax + 1.0f) * hw - 0.5f) - 1.0f, c_hi = floorf((hi[0] / ax + 1.0f) * hw - 0.5f) + 1.0f;
  const float r_lo = ceilf((1.0f - hi[1] / ay) * hh - 0.5f) - 1.0f, r_hi = floorf((1.0f - lo[1] / ay) * hh - 0.5f) + 1.0f;
  if (c_lo > (float)(width - 1) || c_hi < 0.0f || r_lo > (float)(height - 1) || r_hi < 0.0f) { rect[0] = 1; rect[1] = 0; return; }
  rect[0] = (int)fmaxf(c_lo, 0.0f); rect[1] = (int)fminf(c_hi, (float)(width - 1));
  rect[2] = (int)fmaxf(r_lo, 0.0f); rect[3] = (int)fminf(r_hi, (float)(height - 1));
}
