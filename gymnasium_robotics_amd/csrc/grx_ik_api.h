// grx_ik_api.h -- the C ABI of the inverse-kinematics call (include/grx_capi.h grx_sim_ik / grx_sim_ik_layout).  A FRAGMENT of the API section of grx_kernels.hip, included
// behind grx_trimesh_api.h (it uses that section's grx_model, fail and grx_find_table); the kernel is csrc/grx_ik.hip, the argument block and the LDS layout csrc/grx_ik.h.
// The checks that need nothing of the model come first and read nothing of it.
extern "C" int grx_sim_ik(const grx_model* m, const grx_sim_ik_args* r, int n_worlds, void* stream) {
  const std::string w("grx_sim_ik");
  if (!m) return fail(w + ": null model");
  if (!r) return fail(w + ": null argument block");
  if (!r->qpos0 || !r->target_pos || !r->site) return fail(w + ": null qpos0 / target_pos / site");
  if (!r->qpos || !r->err || !r->iters) return fail(w + ": null outputs (qpos, err, iters)");
  if (n_worlds < 1) return fail(w + ": n_worlds < 1");
  if (r->n_sites < 1 || r->n_sites > GRX_IK_MAXSITE) return fail(w + ": n_sites = " + std::to_string(r->n_sites) + " is outside 1 .. " + std::to_string(GRX_IK_MAXSITE));
  if (r->max_iters < 0) return fail(w + ": max_iters < 0");
  if (!(r->damping > 0.0f)) return fail(w + ": damping <= 0");
  if (!(r->tol >= 0.0f)) return fail(w + ": tol < 0");
  if (!(r->max_step > 0.0f)) return fail(w + ": max_step <= 0");
  const GrxModel& g = m->dev;
  if (g.origin[0] != 0.0 || g.origin[1] != 0.0 || g.origin[2] != 0.0) return fail(w + ": the model was compiled with an origin; targets are raw engine coordinates, so compile it in the MJCF's own frame (origin = None)");
  if (g.nshift > 0) return fail(w + ": the model has a per-world shift group (compile_mjcf(shift_body=...)), which only the Adroit task layer feeds");
  for (int k = 0; k < r->n_sites; k++)
    if (r->site[k] < 0 || r->site[k] >= g.nsite) return fail(w + ": site[" + std::to_string(k) + "] = " + std::to_string(r->site[k]) + " is outside [0, nsite)");
  if (g.nmocap > 0 && (!r->mocap_pos || !r->mocap_quat)) return fail(w + ": the model has mocap bodies: null mocap_pos / mocap_quat");
  // each site's chain of dofs (the dofs of its body and of that body's ancestors), from the handle's host copy of the tables grx_model_create packed
  const GrxPackedModel& pm = m->pm;
  auto T = [&](const char* n) { return pm.i.data() + pm.off[grx_find_table(pm, n)]; };
  const int32_t *parent = T("body_parent"), *dof_body = T("dof_bodyid"), *site_body = T("site_bodyid");
  GrxIkArgs a; memset(&a, 0, sizeof(a));
  unsigned long long sel = 0ull;
  for (int d = 0; d < g.nv; d++) if (!r->dof_mask || r->dof_mask[d]) sel |= 1ull << d;
  a.dofsel[0] = (unsigned)sel; a.dofsel[1] = (unsigned)(sel >> 32);
  for (int k = 0; k < r->n_sites; k++) {
    const int sb = site_body[r->site[k]];
    unsigned long long chain = 0ull;
    for (int d = 0; d < g.nv; d++)
      for (int b = sb; b > 0; b = parent[b]) if (dof_body[d] == b) { chain |= 1ull << d; break; }
    chain &= sel;
    a.site[k] = r->site[k]; a.site_body[k] = sb; a.chain_lo[k] = (unsigned)chain; a.chain_hi[k] = (unsigned)(chain >> 32);
  }
  a.body_parent = g.body_parent; a.body_jntadr = g.body_jntadr; a.body_jntnum = g.body_jntnum; a.body_mocapid = g.body_mocapid;
  a.jnt_type = g.jnt_type; a.jnt_qposadr = g.jnt_qposadr; a.jnt_dofadr = g.jnt_dofadr; a.jnt_bodyid = g.jnt_bodyid; a.jnt_limited = g.jnt_limited; a.dof_jntid = g.dof_jntid;
  a.body_order = g.body_order; a.level_adr = g.level_adr;
  a.body_pos = g.body_pos; a.body_quat = g.body_quat; a.jnt_pos = g.jnt_pos; a.jnt_axis = g.jnt_axis; a.jnt_range = g.jnt_range; a.qpos0 = g.qpos0;
  a.site_pos = g.site_pos; a.site_quat = g.site_quat;
  a.nq = g.nq; a.nv = g.nv; a.nbody = g.nbody; a.njnt = g.njnt; a.nmocap = g.nmocap; a.nlevel = g.maxdepth;
  a.qstart = r->qpos0; a.mocap_pos = r->mocap_pos; a.mocap_quat = r->mocap_quat; a.target_pos = r->target_pos; a.target_quat = r->target_quat; a.mask = r->mask;
  a.qpos = r->qpos; a.err = r->err; a.iters = r->iters;
  a.n_sites = r->n_sites; a.rot = r->target_quat ? 1 : 0; a.max_iters = r->max_iters; a.clamp_limits = r->clamp_limits ? 1 : 0;
  a.damping2 = r->damping * r->damping; a.max_step = r->max_step; a.tol = r->tol; a.rot_weight = r->rot_weight;
  a.n_worlds = n_worlds;
  if (grx_tu_ik_wpb(&a, nullptr) < 1) return fail(w + ": one world's working set does not fit the LDS of a workgroup");
  const int e = grx_tu_ik_launch(&a, stream);
  if (e) return fail(w + " launch: " + hipGetErrorString((hipError_t)e));
  return 0;
}
// sizeof(grx_sim_ik_args) and the byte offset of every member, in declaration order: what _native.SimIkStruct must mirror (host only)
extern "C" int grx_sim_ik_layout(long long* out, int cap) {
  const grx_sim_ik_args* z = nullptr;
#define OFF(f) (long long)((const char*)&z->f - (const char*)z)
  const long long v[] = {(long long)sizeof(grx_sim_ik_args), OFF(qpos0), OFF(mocap_pos), OFF(mocap_quat), OFF(target_pos), OFF(target_quat), OFF(mask), OFF(qpos), OFF(err), OFF(iters),
                         OFF(site), OFF(dof_mask), OFF(n_sites), OFF(max_iters), OFF(clamp_limits), OFF(damping), OFF(max_step), OFF(tol), OFF(rot_weight)};
#undef OFF
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  if (out) for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
  return n;
}
