// grx_trimesh_api.h -- the C ABI of the calls that see a mesh geom's triangles (include/grx_capi.h grx_sim_trimesh_create / _destroy, grx_sim_ray_tri, grx_sim_ray_sites_tri,
// grx_sim_render_tri).  A FRAGMENT of the API section of grx_kernels.hip, included behind grx_camera_rgb_api.h; the kernels are csrc/grx_trimesh.hip, the routines and the
// host's check of a hierarchy csrc/grx_trimesh.h.  grx_sim_ray / grx_sim_ray_sites / grx_sim_render stay what they are: their refusals are repeated here, in their order and
// wording, but for the one that does not apply -- a mesh needs no hull to be seen as triangles, so the hull plane cache (grx_ray_cache) is not consulted.
struct grx_trimesh {
  int device = 0, ngeom = 0;
  int32_t *d_nodes = nullptr, *d_adr = nullptr;      // d_adr [3, ngeom]: first node, first triangle, number of nodes
  float* d_tris = nullptr;
  int flags = 0;
};

extern "C" void grx_sim_trimesh_destroy(grx_trimesh* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->d_nodes) (void)hipFree(h->d_nodes);
  if (h->d_adr) (void)hipFree(h->d_adr);
  if (h->d_tris) (void)hipFree(h->d_tris);
  delete h;
}

// The tables are checked FIRST and on the host alone, before the model or the device is looked at: a corrupt hierarchy is refused with its reason wherever the call is made.
extern "C" int grx_sim_trimesh_create(const grx_model* m, const int* nodes, int n_nodes, const float* tris, int n_tris, const int* geom_adr, int n_geom, grx_trimesh** out) {
  const std::string w("grx_sim_trimesh_create");
  if (!out) return fail(w + ": null handle pointer");
  *out = nullptr;
  if (n_nodes < 0 || n_tris < 0 || n_geom < 0) return fail(w + ": a negative count");
  if ((n_nodes > 0 && !nodes) || (n_tris > 0 && !tris) || (n_geom > 0 && !geom_adr)) return fail(w + ": null nodes / tris / geom_adr");
  std::vector<int32_t> count;
  const std::string why = grx_tri_check(nodes, n_nodes, n_tris, geom_adr, n_geom, &count);
  if (!why.empty()) return fail(w + ": " + why);
  if (!m) return fail(w + ": null model");
  const GrxModel& g = m->dev;
  if (n_geom != g.ngeom) return fail(w + ": geom_adr has " + std::to_string(n_geom) + " rows, the model " + std::to_string(g.ngeom) + " geoms");
  const int k_t = grx_find_table(m->pm, "geom_type");
  if (k_t < 0 || m->pm.cnt[k_t] < n_geom) return fail(w + ": the model holds no geom_type table");
  const int32_t* type = m->pm.i.data() + m->pm.off[k_t];
  for (int i = 0; i < n_geom; i++)
    if ((type[i] == 7) != (geom_adr[2 * i] >= 0)) return fail(w + ": geom " + std::to_string(i) + (type[i] == 7 ? " is a mesh without a hierarchy" : " is no mesh but has a hierarchy"));
  std::vector<int32_t> adr(3 * (size_t)(n_geom > 0 ? n_geom : 1), -1);
  for (int i = 0; i < n_geom; i++) { adr[i] = geom_adr[2 * i]; adr[n_geom + i] = geom_adr[2 * i + 1]; adr[2 * (size_t)n_geom + i] = count[i]; }
  grx_trimesh* h = new grx_trimesh;
  h->device = m->device; h->ngeom = n_geom;
  // A/B switches of the render kernel (profiles/trimesh_render.json): GRX_TRIMESH_WALK=lane walks a mesh lane by lane, GRX_TRIMESH_WINDOW=0 reads every node from global memory
  if (getenv("GRX_TRIMESH_WALK") && std::string(getenv("GRX_TRIMESH_WALK")) == "lane") h->flags |= GRX_TRI_PER_LANE;
  if (getenv("GRX_TRIMESH_WINDOW") && std::string(getenv("GRX_TRIMESH_WINDOW")) == "0") h->flags |= GRX_TRI_NO_WINDOW;
  const size_t bn = sizeof(int32_t) * GRX_TRI_NODE * (size_t)(n_nodes > 0 ? n_nodes : 1), bt = sizeof(float) * GRX_TRI_WORDS * (size_t)(n_tris > 0 ? n_tris : 1);
  bool ok = hipSetDevice(m->device) == hipSuccess && hipMalloc(&h->d_nodes, bn) == hipSuccess && hipMalloc(&h->d_tris, bt) == hipSuccess && hipMalloc(&h->d_adr, sizeof(int32_t) * adr.size()) == hipSuccess;
  ok = ok && (n_nodes == 0 || hipMemcpy(h->d_nodes, nodes, sizeof(int32_t) * GRX_TRI_NODE * (size_t)n_nodes, hipMemcpyHostToDevice) == hipSuccess);
  ok = ok && (n_tris == 0 || hipMemcpy(h->d_tris, tris, sizeof(float) * GRX_TRI_WORDS * (size_t)n_tris, hipMemcpyHostToDevice) == hipSuccess);
  ok = ok && hipMemcpy(h->d_adr, adr.data(), sizeof(int32_t) * adr.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { grx_sim_trimesh_destroy(h); return fail(w + ": allocation or upload of the hierarchy failed"); }
  *out = h;
  return 0;
}

static int grx_trimesh_args(const std::string& w, const grx_model* m, const grx_trimesh* h, GrxTriArgs* t) {
  if (!h) return fail(w + ": null triangle handle");
  if (h->device != m->device || h->ngeom != m->dev.ngeom) return fail(w + ": the triangle handle was made for another model");
  t->nodes = h->d_nodes; t->tris = h->d_tris; t->geom_adr = h->d_adr; t->flags = h->flags;
  return 0;
}

static int grx_sim_ray_tri_impl(const char* who, const grx_model* m, const grx_sim_rays* r, const grx_trimesh* h, int n_worlds, int n_rays, void* stream, bool sites) {
  const std::string w(who);
  if (!m) return fail(w + ": null model");
  if (!r) return fail(w + ": null ray block");
  if (!r->xpos || !r->xquat) return fail(w + ": null body poses (xpos, xquat)");
  if (!r->dist) return fail(w + ": null dist buffer");
  if (n_worlds < 1) return fail(w + ": n_worlds < 1");
  if (n_rays < 1) return fail(w + ": n_rays < 1");
  if (sites) {
    if (!r->site_xpos || !r->site_xmat) return fail(w + ": null site poses (site_xpos, site_xmat)");
    if (!r->ray_site || !r->local_dir) return fail(w + ": null ray_site / local_dir");
  } else if (!r->origin || !r->direction) return fail(w + ": null origin / direction");
  const GrxModel& g = m->dev;
  if (g.origin[0] != 0.0 || g.origin[1] != 0.0 || g.origin[2] != 0.0) return fail(w + ": the model was compiled with an origin; rays are cast in raw engine coordinates, so compile it in the MJCF's own frame (origin = None)");
  if (g.nshift > 0) return fail(w + ": the model has a per-world shift group (compile_mjcf(shift_body=...)), which only the Adroit task layer feeds");
  const int* d_sites = nullptr;
  if (sites) {
    for (int k = 0; k < n_rays; k++)
      if (r->ray_site[k] < 0 || r->ray_site[k] >= g.nsite) return fail(w + ": ray_site[" + std::to_string(k) + "] = " + std::to_string(r->ray_site[k]) + " is outside [0, nsite)");
  }
  GrxTriArgs t;
  if (grx_trimesh_args(w, m, h, &t)) return -1;
  if (sites && grx_ray_site_list(m, r->ray_site, n_rays, &d_sites)) return -1;
  GrxRayArgs a; memset(&a, 0, sizeof(a));      // plane_adr / plane_num / planes stay NULL: the kernel stages the hierarchy's table in their place
  a.geom_type = g.geom_type; a.geom_bodyid = g.geom_bodyid; a.site_bodyid = g.site_bodyid;
  a.geom_pos = g.geom_pos; a.geom_quat = g.geom_quat; a.geom_size = g.geom_size; a.geom_rbound = g.geom_rbound;
  a.ngeom = g.ngeom; a.nbody = g.nbody; a.nsite = g.nsite;
  a.xpos = r->xpos; a.xquat = r->xquat; a.origin = r->origin; a.direction = r->direction; a.site_xpos = r->site_xpos; a.site_xmat = r->site_xmat; a.local_dir = r->local_dir;
  a.ray_site = d_sites; a.exclude_body = r->exclude_body; a.mask = r->mask; a.dist = r->dist; a.geom = r->geom;
  a.max_dist = r->max_dist; a.include_static = r->include_static; a.exclude_site_body = sites ? r->exclude_site_body : 0; a.sites = sites ? 1 : 0;
  a.n_worlds = n_worlds; a.n_rays = n_rays;
  const int e = grx_tu_trimesh_rays_launch(&a, &t, stream);
  if (e) return fail(w + " launch: " + hipGetErrorString((hipError_t)e));
  return 0;
}
extern "C" int grx_sim_ray_tri(const grx_model* m, const grx_sim_rays* r, const grx_trimesh* h, int n_worlds, int n_rays, void* stream) {
  return grx_sim_ray_tri_impl("grx_sim_ray_tri", m, r, h, n_worlds, n_rays, stream, false);
}
extern "C" int grx_sim_ray_sites_tri(const grx_model* m, const grx_sim_rays* r, const grx_trimesh* h, int n_worlds, int n_rays, void* stream) {
  return grx_sim_ray_tri_impl("grx_sim_ray_sites_tri", m, r, h, n_worlds, n_rays, stream, true);
}

extern "C" int grx_sim_render_tri(const grx_model* m, const grx_sim_cameras* c, const grx_trimesh* h, int n_worlds, int n_cams, int height, int width, void* stream) {
  const std::string w("grx_sim_render_tri");
  if (!m) return fail(w + ": null model");
  if (!c) return fail(w + ": null camera block");
  if (!c->xpos || !c->xquat) return fail(w + ": null body poses (xpos, xquat)");
  if (!c->depth) return fail(w + ": null depth buffer");
  if (n_worlds < 1) return fail(w + ": n_worlds < 1");
  if (n_cams < 1 || n_cams > GRX_CAM_MAX) return fail(w + ": n_cams = " + std::to_string(n_cams) + " is outside 1 .. " + std::to_string(GRX_CAM_MAX));
  if (height < 1 || height > GRX_CAM_MAX_SIDE || width < 1 || width > GRX_CAM_MAX_SIDE)
    return fail(w + ": height x width = " + std::to_string(height) + " x " + std::to_string(width) + " is outside 1 .. " + std::to_string(GRX_CAM_MAX_SIDE));
  const bool posed = c->pose_pos != nullptr;
  if (posed && !c->pose_mat) return fail(w + ": pose_pos without pose_mat");
  if (!posed && (!c->cam_body || !c->cam_pos || !c->cam_quat)) return fail(w + ": null camera poses (cam_body, cam_pos, cam_quat, or pose_pos, pose_mat)");
  if (!c->cam_fovy) return fail(w + ": null cam_fovy");
  const GrxModel& g = m->dev;
  if (g.origin[0] != 0.0 || g.origin[1] != 0.0 || g.origin[2] != 0.0) return fail(w + ": the model was compiled with an origin; cameras see raw engine coordinates, so compile it in the MJCF's own frame (origin = None)");
  if (g.nshift > 0) return fail(w + ": the model has a per-world shift group (compile_mjcf(shift_body=...)), which only the Adroit task layer feeds");
  GrxCamArgs a; memset(&a, 0, sizeof(a));
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
  GrxTriArgs t;
  if (grx_trimesh_args(w, m, h, &t)) return -1;
  a.geom_type = g.geom_type; a.geom_bodyid = g.geom_bodyid;      // (plane_adr / plane_num / planes stay NULL, as in the ray calls above)
  a.geom_pos = g.geom_pos; a.geom_quat = g.geom_quat; a.geom_size = g.geom_size; a.geom_rbound = g.geom_rbound;
  a.ngeom = g.ngeom; a.nbody = g.nbody;
  a.xpos = c->xpos; a.xquat = c->xquat; a.pose_pos = c->pose_pos; a.pose_mat = c->pose_mat;
  a.mask = c->mask; a.depth = c->depth; a.seg = c->seg;
  a.max_dist = c->max_dist; a.include_static = c->include_static; a.exclude_own_body = c->exclude_own_body;
  a.flags = (c->no_binning ? GRX_CAM_NO_BINNING : 0) | (c->tile_16x4 ? GRX_CAM_TILE_16X4 : 0);
  a.n_worlds = n_worlds; a.n_cams = n_cams; a.height = height; a.width = width;
  const int e = grx_tu_trimesh_render_launch(&a, &t, stream);
  if (e) return fail(w + " launch: " + hipGetErrorString((hipError_t)e));
  return 0;
}
