// grx_rays_api.h -- the C ABI of the ray calls (include/grx_capi.h grx_sim_ray / grx_sim_ray_sites / grx_sim_rays_layout).  A FRAGMENT of the API section of grx_kernels.hip
// (it uses that section's grx_model, fail and HIP_OK), as grx_sim_params_api.h is; the kernel is csrc/grx_rays.hip, the routines csrc/grx_rays.h.
static_assert(sizeof(((grx_sim_rays*)0)->mask) == sizeof(void*), "grx_sim_rays holds pointers");

// The hulls' face planes of the handle, derived once, under the handle's lock, when it first serves a ray call (a blocking upload, that one time): planes [P, 4] and per geom
// (first plane, planes).  Two geoms of one mesh share their planes.
static int grx_ray_cache(const grx_model* m) {
  std::lock_guard<std::mutex> lk(m->ray_mu);
  if (m->ray_ready) return 0;
  const GrxPackedModel& pm = m->pm;
  const int ngeom = m->dev.ngeom;
  auto T = [&](const char* n) { return grx_find_table(pm, n); };
  const int k_adr = T("geom_hulladr"), k_num = T("geom_hullnum"), k_v = T("mesh_vert"), k_aa = T("mesh_adjadr"), k_an = T("mesh_adjnum"), k_a = T("mesh_adj"), k_t = T("geom_type");
  std::vector<float> planes;
  std::vector<int32_t> adr(2 * (size_t)(ngeom > 0 ? ngeom : 1), 0);
  if (k_adr >= 0 && k_num >= 0 && k_v >= 0 && k_aa >= 0 && k_an >= 0 && k_a >= 0 && k_t >= 0) {
    const int32_t *hadr = pm.i.data() + pm.off[k_adr], *hnum = pm.i.data() + pm.off[k_num], *aa = pm.i.data() + pm.off[k_aa], *an = pm.i.data() + pm.off[k_an], *ad = pm.i.data() + pm.off[k_a];
    const int32_t* type = pm.i.data() + pm.off[k_t];
    const int nvert = pm.cnt[k_v] / 3, nh = pm.cnt[k_adr] < pm.cnt[k_num] ? pm.cnt[k_adr] : pm.cnt[k_num];
    for (int g = 0; g < ngeom && g < nh && g < pm.cnt[k_t]; g++) {
      if (type[g] != 7) continue;
      // the compiled model keeps a mesh's full hull only when the mesh has a candidate pair with a convex geom (geom_hulladr / geom_hullnum); one that meets planes only, or
      // nothing, has none, and a ray could not see it: refuse the call rather than pass through it
      if (hadr[g] < 0 || hnum[g] < 4 || hadr[g] + hnum[g] > nvert || hadr[g] + hnum[g] > pm.cnt[k_aa] || hadr[g] + hnum[g] > pm.cnt[k_an])
        return fail("grx_sim_ray: geom " + std::to_string(g) + " is a mesh without a full hull in the compiled model (it has no candidate pair with a sphere, capsule, ellipsoid, cylinder, box or mesh), so rays cannot see it");
      bool shared = false;
      for (int h = 0; h < g && !shared; h++)
        if (type[h] == 7 && hadr[h] == hadr[g] && hnum[h] == hnum[g] && adr[ngeom + h] > 0) { adr[g] = adr[h]; adr[ngeom + g] = adr[ngeom + h]; shared = true; }
      if (shared) continue;
      bool ok = true;      // the adjacency stays inside its table
      for (int v = 0; v < hnum[g] && ok; v++) ok = aa[hadr[g] + v] >= 0 && an[hadr[g] + v] >= 0 && aa[hadr[g] + v] + an[hadr[g] + v] <= pm.cnt[k_a];
      if (!ok) return fail("grx_sim_ray: the hull adjacency of geom " + std::to_string(g) + " leaves its table");
      std::vector<double> vert(3 * (size_t)hnum[g]);
      for (size_t k = 0; k < vert.size(); k++) vert[k] = pm.f[pm.off[k_v] + 3 * (size_t)hadr[g] + k];
      adr[g] = (int32_t)(planes.size() / 4);
      adr[ngeom + g] = grx_hull_planes(vert.data(), hnum[g], aa + hadr[g], an + hadr[g], ad, &planes);
      if (adr[ngeom + g] < 4) return fail("grx_sim_ray: the hull of geom " + std::to_string(g) + " has no volume (fewer than four face planes)");
    }
  }
  if (planes.empty()) planes.assign(4, 0.0f);
  HIP_OK(hipSetDevice(m->device));
  float* dp = nullptr; int32_t* da = nullptr;
  HIP_OK(hipMalloc(&dp, sizeof(float) * planes.size()));
  if (hipMalloc(&da, sizeof(int32_t) * adr.size()) != hipSuccess) { (void)hipFree(dp); return fail("grx_sim_ray: hipMalloc of the hull plane ranges failed"); }
  if (hipMemcpy(dp, planes.data(), sizeof(float) * planes.size(), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(da, adr.data(), sizeof(int32_t) * adr.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(dp); (void)hipFree(da);
    return fail("grx_sim_ray: upload of the hull planes failed");
  }
  m->d_ray_planes = dp; m->d_ray_adr = da; m->ray_ready = true;
  return 0;
}

// the device copy of a ray_site list (host, n entries, checked by the caller): made once per distinct list (one blocking upload) and kept with the handle, so a lidar that casts
// from the same sites every step uploads them once and no later launch waits for a copy.  The handle keeps the 64 most recent lists.
static int grx_ray_site_list(const grx_model* m, const int* host, int n, const int** out) {
  std::lock_guard<std::mutex> lk(m->ray_mu);
  std::vector<int> key(host, host + n);
  for (auto& e : m->ray_sites) if (e.first == key) { *out = e.second; return 0; }
  HIP_OK(hipSetDevice(m->device));
  if (m->ray_sites.size() >= 64) {      // the oldest list goes: hipFree waits for the launches that may still read it
    (void)hipFree(m->ray_sites.front().second);
    m->ray_sites.erase(m->ray_sites.begin());
  }
  int* d = nullptr;
  HIP_OK(hipMalloc(&d, sizeof(int) * (size_t)n));
  if (hipMemcpy(d, host, sizeof(int) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return fail("grx_sim_ray_sites: upload of ray_site failed"); }
  m->ray_sites.emplace_back(std::move(key), d);
  *out = d;
  return 0;
}

static int grx_sim_ray_impl(const char* who, const grx_model* m, const grx_sim_rays* r, int n_worlds, int n_rays, void* stream, bool sites) {
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
  if (grx_ray_cache(m)) return -1;
  if (sites && grx_ray_site_list(m, r->ray_site, n_rays, &d_sites)) return -1;
  GrxRayArgs a; memset(&a, 0, sizeof(a));
  a.geom_type = g.geom_type; a.geom_bodyid = g.geom_bodyid; a.site_bodyid = g.site_bodyid; a.plane_adr = m->d_ray_adr; a.plane_num = m->d_ray_adr + g.ngeom;
  a.geom_pos = g.geom_pos; a.geom_quat = g.geom_quat; a.geom_size = g.geom_size; a.geom_rbound = g.geom_rbound; a.planes = m->d_ray_planes;
  a.ngeom = g.ngeom; a.nbody = g.nbody; a.nsite = g.nsite;
  a.xpos = r->xpos; a.xquat = r->xquat; a.origin = r->origin; a.direction = r->direction; a.site_xpos = r->site_xpos; a.site_xmat = r->site_xmat; a.local_dir = r->local_dir;
  a.ray_site = d_sites; a.exclude_body = r->exclude_body; a.mask = r->mask; a.dist = r->dist; a.geom = r->geom;
  a.max_dist = r->max_dist; a.include_static = r->include_static; a.exclude_site_body = sites ? r->exclude_site_body : 0; a.sites = sites ? 1 : 0;
  a.n_worlds = n_worlds; a.n_rays = n_rays;
  const int e = grx_tu_rays_launch(&a, stream);
  if (e) return fail(w + " launch: " + hipGetErrorString((hipError_t)e));
  return 0;
}
extern "C" int grx_sim_ray(const grx_model* m, const grx_sim_rays* r, int n_worlds, int n_rays, void* stream) { return grx_sim_ray_impl("grx_sim_ray", m, r, n_worlds, n_rays, stream, false); }
extern "C" int grx_sim_ray_sites(const grx_model* m, const grx_sim_rays* r, int n_worlds, int n_rays, void* stream) { return grx_sim_ray_impl("grx_sim_ray_sites", m, r, n_worlds, n_rays, stream, true); }
// sizeof(grx_sim_rays) and the byte offset of every member, in declaration order: what _native.SimRaysStruct must mirror (host only)
extern "C" int grx_sim_rays_layout(long long* out, int cap) {
  const grx_sim_rays* z = nullptr;
#define OFF(f) (long long)((const char*)&z->f - (const char*)z)
  const long long v[] = {(long long)sizeof(grx_sim_rays), OFF(xpos), OFF(xquat), OFF(origin), OFF(direction), OFF(site_xpos), OFF(site_xmat), OFF(ray_site), OFF(local_dir), OFF(exclude_body),
                         OFF(mask), OFF(dist), OFF(geom), OFF(max_dist), OFF(include_static), OFF(exclude_site_body)};
#undef OFF
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  if (out) for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
  return n;
}
