// grx_camera_rgb_api.h -- the C ABI of the colour / surface-normal camera call (include/grx_capi.h grx_sim_render_rgb / grx_sim_shade_layout).  A FRAGMENT of the API section
// of grx_kernels.hip, included behind grx_camera_api.h; the kernel is csrc/grx_camera_rgb.hip.  grx_sim_render stays what it is: its refusals are repeated here, in its order
// and its words, rather than moved out of it.
extern "C" int grx_sim_render_rgb(const grx_model* m, const grx_sim_cameras* c, const grx_sim_shade* sh, int n_worlds, int n_cams, int height, int width, void* stream) {
  const std::string w("grx_sim_render_rgb");
  if (!m) return fail(w + ": null model");
  if (!c) return fail(w + ": null camera block");
  if (!sh) return fail(w + ": null shade block");
  if (!c->xpos || !c->xquat) return fail(w + ": null body poses (xpos, xquat)");
  if (!c->depth) return fail(w + ": null depth buffer");
  if (!sh->rgba && !sh->normal) return fail(w + ": null rgba and normal buffers (one of them at least)");
  if (sh->rgba && !sh->colors) return fail(w + ": rgba without colors");
  if (n_worlds < 1) return fail(w + ": n_worlds < 1");
  if (n_cams < 1 || n_cams > GRX_CAM_MAX) return fail(w + ": n_cams = " + std::to_string(n_cams) + " is outside 1 .. " + std::to_string(GRX_CAM_MAX));
  if (height < 1 || height > GRX_CAM_MAX_SIDE || width < 1 || width > GRX_CAM_MAX_SIDE)
    return fail(w + ": height x width = " + std::to_string(height) + " x " + std::to_string(width) + " is outside 1 .. " + std::to_string(GRX_CAM_MAX_SIDE));
  const bool posed = c->pose_pos != nullptr;
  if (posed && !c->pose_mat) return fail(w + ": pose_pos without pose_mat");
  if (!posed && (!c->cam_body || !c->cam_pos || !c->cam_quat)) return fail(w + ": null camera poses (cam_body, cam_pos, cam_quat, or pose_pos, pose_mat)");
  if (!c->cam_fovy) return fail(w + ": null cam_fovy");
  const float terms[3] = {sh->ambient, sh->diffuse, sh->sun_diffuse};
  for (float x : terms)
    if (!(x >= 0.0f && x < INFINITY)) return fail(w + ": ambient, diffuse and sun_diffuse must be finite and >= 0");
  for (float x : sh->background)
    if (!(std::fabs(x) < INFINITY)) return fail(w + ": background is not finite");
  const GrxModel& g = m->dev;
  if (g.origin[0] != 0.0 || g.origin[1] != 0.0 || g.origin[2] != 0.0) return fail(w + ": the model was compiled with an origin; cameras see raw engine coordinates, so compile it in the MJCF's own frame (origin = None)");
  if (g.nshift > 0) return fail(w + ": the model has a per-world shift group (compile_mjcf(shift_body=...)), which only the Adroit task layer feeds");
  GrxCamRgbArgs s; memset(&s, 0, sizeof(s));
  GrxCamArgs& a = s.c;
  if (sh->sun_diffuse > 0.0f) {      // the sun is read only then: made unit here, in fp64
    double n = 0.0;
    for (int i = 0; i < 3; i++) n += (double)sh->sun[i] * sh->sun[i];
    if (!(n > 1e-20) || !(n < 1e30)) return fail(w + ": sun is zero or not finite");
    for (int i = 0; i < 3; i++) s.light.sun[i] = (float)(sh->sun[i] / std::sqrt(n));
    s.light.has_sun = 1;
  }
  for (int k = 0; k < n_cams; k++) {
    const float f = c->cam_fovy[k];
    if (!(f > 0.0f && f < 180.0f)) return fail(w + ": cam_fovy[" + std::to_string(k) + "] = " + std::to_string(f) + " is outside (0, 180) degrees");
    a.cam_tan[k] = (float)std::tan(0.5 * (double)f * 3.14159265358979323846 / 180.0);
    a.cam_body[k] = -1;
    a.cam_quat[k][0] = 1.0f;
    a.exclude_body[k] = c->exclude_body ? c->exclude_body[k] : -1;
    if (posed) continue;
    if (c->cam_body[k] < 0 || c->cam_body[k] >= g.nbody) return fail(w + ": cam_body[" + std::to_string(k) + "] = " + std::to_string(c->cam_body[k]) + " is outside [0, nbody)");
    a.cam_body[k] = c->cam_body[k];
    double n = 0.0;
    for (int i = 0; i < 4; i++) n += (double)c->cam_quat[4 * k + i] * c->cam_quat[4 * k + i];
    if (!(n > 1e-20) || !(n < 1e30)) return fail(w + ": cam_quat[" + std::to_string(k) + "] is zero or not finite");
    for (int i = 0; i < 4; i++) a.cam_quat[k][i] = (float)(c->cam_quat[4 * k + i] / std::sqrt(n));
    for (int i = 0; i < 3; i++) a.cam_pos[k][i] = c->cam_pos[3 * k + i];
  }
  if (grx_ray_cache(m)) return -1;
  a.geom_type = g.geom_type; a.geom_bodyid = g.geom_bodyid; a.plane_adr = m->d_ray_adr; a.plane_num = m->d_ray_adr + g.ngeom;
  a.geom_pos = g.geom_pos; a.geom_quat = g.geom_quat; a.geom_size = g.geom_size; a.geom_rbound = g.geom_rbound; a.planes = m->d_ray_planes;
  a.ngeom = g.ngeom; a.nbody = g.nbody;
  a.xpos = c->xpos; a.xquat = c->xquat; a.pose_pos = c->pose_pos; a.pose_mat = c->pose_mat;
  a.mask = c->mask; a.depth = c->depth; a.seg = c->seg;
  a.max_dist = c->max_dist; a.include_static = c->include_static; a.exclude_own_body = c->exclude_own_body;
  a.flags = (c->no_binning ? GRX_CAM_NO_BINNING : 0) | (c->tile_16x4 ? GRX_CAM_TILE_16X4 : 0);
  a.n_worlds = n_worlds; a.n_cams = n_cams; a.height = height; a.width = width;
  s.rgba = sh->rgba; s.normal = sh->normal; s.colors = sh->colors; s.colors_per_world = sh->colors_per_world != 0;
  s.light.ambient = sh->ambient; s.light.diffuse = sh->diffuse; s.light.sun_diffuse = sh->sun_diffuse;
  s.background = grx_shade_pack(sh->background[0], sh->background[1], sh->background[2], 0u);
  const int e = grx_tu_camera_rgb_launch(&s, stream);
  if (e) return fail(w + " launch: " + hipGetErrorString((hipError_t)e));
  return 0;
}
// sizeof(grx_sim_shade) and the byte offset of every member, in declaration order: what _native.SimShadeStruct must mirror (host only)
extern "C" int grx_sim_shade_layout(long long* out, int cap) {
  const grx_sim_shade* z = nullptr;
#define OFF(f) (long long)((const char*)&z->f - (const char*)z)
  const long long v[] = {(long long)sizeof(grx_sim_shade), OFF(rgba), OFF(normal), OFF(colors), OFF(colors_per_world), OFF(ambient), OFF(diffuse), OFF(sun), OFF(sun_diffuse), OFF(background)};
#undef OFF
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  if (out) for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
  return n;
}
