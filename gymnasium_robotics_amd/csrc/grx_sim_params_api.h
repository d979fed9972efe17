// grx_sim_params_api.h -- the host side of the per-world model parameters (include/grx_capi.h grx_sim_params_*): included by the API unit of grx_kernels.hip, behind
// grx_sim_step_impl.  The device side and the layout of an object: csrc/grx_sim_params.h.
#pragma once

static const char* const g_param_names[GRX_NPT] = {
#define X(n) #n,
  GRX_PARAM_TABLES(X)
#undef X
  "gravity"};
static int grx_param_id(const char* name) {
  for (int t = 0; t < GRX_NPT; t++) if (!strcmp(name, g_param_names[t])) return t;
  return -1;
}
static std::string grx_param_name_list() {
  std::string s;
  for (int t = 0; t < GRX_NPT; t++) { if (t) s += ", "; s += g_param_names[t]; }
  return s;
}
// the named-table member of a descriptor
static const float** grx_param_member(GrxModel* g, int t) {
  switch (t) {
#define X(n) case GRX_PT_##n: return &g->n;
    GRX_PARAM_TABLES(X)
#undef X
    default: return nullptr;
  }
}
static const float** grx_param_record_member(GrxModel* g, int kind) {
  return kind == GRX_PR_DOF ? &g->recf_dof : kind == GRX_PR_MPAIR ? &g->recf_mpair : kind == GRX_PR_JNT ? &g->recf_jnt : kind == GRX_PR_ACT ? &g->recf_act : &g->recf_pair;
}
static int grx_param_record_offset(const GrxPackedModel& pm, int kind) {
  return kind == GRX_PR_DOF ? pm.rec.f_dof : kind == GRX_PR_MPAIR ? pm.rec.f_mpair : kind == GRX_PR_JNT ? pm.rec.f_jnt : kind == GRX_PR_ACT ? pm.rec.f_act : pm.rec.f_pair;
}
// entity counts of the record kinds, as grx_build_records takes them
static GrxParamCounts grx_param_counts(const GrxPackedModel& pm) {
  auto C = [&](const char* n) { const int k = grx_find_table(pm, n); return k >= 0 ? pm.cnt[k] : 0; };
  GrxParamCounts c;
  c.n[GRX_PR_DOF] = pm.proto.nv; c.n[GRX_PR_MPAIR] = C("mpair_i"); c.n[GRX_PR_JNT] = pm.proto.njnt; c.n[GRX_PR_ACT] = pm.proto.nu; c.n[GRX_PR_PAIR] = C("pair_geom1");
  c.has_dofprm = (C("dof_solref") >= 2 * pm.proto.nv && C("dof_solimp") >= 5 * pm.proto.nv) ? 1 : 0;
  return c;
}
static int grx_param_table_count(const GrxPackedModel& pm, int t) {
  if (t == GRX_PT_gravity) return 3;
  const int k = grx_find_table(pm, g_param_names[t]);
  return k >= 0 ? pm.cnt[k] : 0;
}

struct grx_sim_params {
  const grx_model* model = nullptr; const grx_model* large = nullptr;
  int n = 0, device = 0, stride = 0;
  int named[GRX_NPT] = {0}, cnt[GRX_NPT] = {0}, stage_off[GRX_NPT] = {0}, live_off[GRX_NPT] = {0}, rec_off[GRX_NPR] = {0};
  float* d_stage = nullptr; float* d_live = nullptr;
  GrxModel* d_desc = nullptr; GrxModel* d_desc_large = nullptr;
  int* d_bits = nullptr;
  GrxParamCommit args;
};

extern "C" int grx_sim_params_destroy(grx_sim_params* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  if (p->d_stage) (void)hipFree(p->d_stage);
  if (p->d_live) (void)hipFree(p->d_live);
  if (p->d_desc) (void)hipFree(p->d_desc);
  if (p->d_desc_large) (void)hipFree(p->d_desc_large);
  if (p->d_bits) (void)hipFree(p->d_bits);
  delete p;
  return 0;
}

static int grx_sim_params_create_impl(grx_sim_params* p) {
  const grx_model* m = p->model;
  const GrxPackedModel& pm = m->pm;
  const int N = p->n;
  const GrxParamCounts counts = grx_param_counts(pm);
  auto pad4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
  // layout: the stage rows table by table ([N, cnt] each); a world's live block = its rows, then its private records
  size_t stage_words = 0; int kinds = 0; size_t live = 0;
  for (int t = 0; t < GRX_NPT; t++) {
    if (!p->named[t]) continue;
    p->cnt[t] = grx_param_table_count(pm, t);
    p->stage_off[t] = (int)stage_words; stage_words = pad4(stage_words + (size_t)N * p->cnt[t]);
    kinds |= grx_param_record_deps(t);
    if (t != GRX_PT_gravity) { p->live_off[t] = (int)live; live = pad4(live + p->cnt[t]); }
  }
  for (int k = 0; k < GRX_NPR; k++) {
    p->rec_off[k] = -1;
    if (!((kinds >> k) & 1) || counts.n[k] == 0) { kinds &= ~(1 << k); continue; }
    p->rec_off[k] = (int)live; live = pad4(live + (size_t)counts.n[k] * grx_param_record_words(k));
  }
  p->stride = (int)(live > 0 ? live : 4);
  HIP_OK(hipSetDevice(p->device));
  HIP_OK(hipMalloc(&p->d_stage, sizeof(float) * (stage_words + 4)));
  HIP_OK(hipMalloc(&p->d_live, sizeof(float) * ((size_t)N * p->stride + 4)));
  HIP_OK(hipMalloc(&p->d_desc, sizeof(GrxModel) * (size_t)N));
  if (p->large) HIP_OK(hipMalloc(&p->d_desc_large, sizeof(GrxModel) * (size_t)N));
  HIP_OK(hipMalloc(&p->d_bits, sizeof(int) * (size_t)N));
  HIP_OK(hipMemset(p->d_bits, 0, sizeof(int) * (size_t)N));
  // nominal start: every world's stage rows and live rows hold the model's own fp32 values, its private records are copies of the shared ones
  std::vector<float> stage(stage_words, 0.0f), block((size_t)p->stride, 0.0f), all((size_t)N * p->stride);
  for (int t = 0; t < GRX_NPT; t++) {
    if (!p->named[t]) continue;
    const float* nom = t == GRX_PT_gravity ? pm.proto.gravity : pm.f.data() + pm.off[grx_find_table(pm, g_param_names[t])];
    for (int w = 0; w < N; w++) memcpy(stage.data() + p->stage_off[t] + (size_t)w * p->cnt[t], nom, sizeof(float) * p->cnt[t]);
    if (t != GRX_PT_gravity) memcpy(block.data() + p->live_off[t], nom, sizeof(float) * p->cnt[t]);
  }
  for (int k = 0; k < GRX_NPR; k++)
    if (p->rec_off[k] >= 0) memcpy(block.data() + p->rec_off[k], pm.f.data() + grx_param_record_offset(pm, k), sizeof(float) * (size_t)counts.n[k] * grx_param_record_words(k));
  for (int w = 0; w < N; w++) memcpy(all.data() + (size_t)w * p->stride, block.data(), sizeof(float) * p->stride);
  if (stage_words) HIP_OK(hipMemcpy(p->d_stage, stage.data(), sizeof(float) * stage_words, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(p->d_live, all.data(), sizeof(float) * all.size(), hipMemcpyHostToDevice));
  // the descriptors: the handle's own, with the named tables and their records redirected to the world's live block
  for (int pass = 0; pass < 2; pass++) {
    const grx_model* h = pass ? p->large : m;
    if (!h) continue;
    std::vector<GrxModel> desc((size_t)N, h->dev);
    for (int w = 0; w < N; w++) {
      const float* base = p->d_live + (size_t)w * p->stride;
      for (int t = 0; t < GRX_NPT; t++) if (p->named[t] && t != GRX_PT_gravity) *grx_param_member(&desc[w], t) = base + p->live_off[t];
      for (int k = 0; k < GRX_NPR; k++) if (p->rec_off[k] >= 0) *grx_param_record_member(&desc[w], k) = base + p->rec_off[k];
    }
    HIP_OK(hipMemcpy(pass ? p->d_desc_large : p->d_desc, desc.data(), sizeof(GrxModel) * (size_t)N, hipMemcpyHostToDevice));
    int e;
    const int bytes = h->words * 4 + h->lds_pad;
    for (const GrxSimUnit& u : g_sim_units)   // the parameter twins of the stepper's units: no descriptor, no slot
      if (u.prm && (e = u.prepare(nullptr, bytes, 0)) != 0) return fail(std::string("grx_sim_params_create (kernels with per-world parameters): ") + hipGetErrorString((hipError_t)e));
  }
  GrxParamCommit& a = p->args;
  memset(&a, 0, sizeof(a));
  for (int t = 0; t < GRX_NPT; t++) {
    if (!p->named[t]) continue;
    a.stage[t] = p->d_stage + p->stage_off[t]; a.cnt[t] = p->cnt[t]; a.live_off[t] = p->live_off[t];
    a.nominal[t] = t == GRX_PT_gravity ? nullptr : m->d_f + pm.off[grx_find_table(pm, g_param_names[t])];
  }
  a.live = p->d_live; a.stride = p->stride; a.desc = p->d_desc; a.desc_large = p->d_desc_large;
  a.jnt_limited = m->dev.jnt_limited; a.anydamp = m->dev.anydamp; a.kinds = kinds; a.counts = counts;
  a.bits = p->d_bits; a.n_worlds = N;
  return 0;
}

extern "C" int grx_sim_params_create(const grx_model* model, const grx_model* model_large, int n_worlds, const char* const* names, int n_names, grx_sim_params** out) {
  if (!model || !out) return fail("grx_sim_params_create: null argument (model, out)");
  if (n_names < 0 || (n_names > 0 && !names)) return fail("grx_sim_params_create: null names");
  if (n_worlds < 1) return fail("grx_sim_params_create: n_worlds < 1");
  int named[GRX_NPT] = {0};
  for (int k = 0; k < n_names; k++) {
    if (!names[k]) return fail("grx_sim_params_create: null name");
    const int t = grx_param_id(names[k]);
    if (t < 0) return fail(std::string("grx_sim_params_create: no per-world parameter named '") + names[k] + "'; the parameters are " + grx_param_name_list());
    if (named[t]) return fail(std::string("grx_sim_params_create: '") + names[k] + "' is named twice");
    named[t] = 1;
  }
  if (model_large) {
    if (model_large == model) return fail("grx_sim_params_create: the large-table handle is the model itself");
    if (model_large->device != model->device) return fail("grx_sim_params_create: the two handles live on different devices");
    const GrxPackedModel &a = model->pm, &b = model_large->pm;
    bool same = a.cnt.size() == b.cnt.size() && a.proto.nv == b.proto.nv && a.proto.njnt == b.proto.njnt && a.proto.nu == b.proto.nu && a.proto.nbody == b.proto.nbody;
    for (size_t k = 0; same && k < a.cnt.size(); k++) same = a.cnt[k] == b.cnt[k] && a.name[k] == b.name[k];
    if (!same) return fail("grx_sim_params_create: the large-table handle's table shapes differ from the model's (it must be the same model with other capacities)");
  }
  grx_sim_params* p = new grx_sim_params();
  p->model = model; p->large = model_large; p->n = n_worlds; p->device = model->device;
  memcpy(p->named, named, sizeof(named));
  if (grx_sim_params_create_impl(p)) { grx_sim_params_destroy(p); return -1; }
  *out = p;
  return 0;
}

extern "C" int grx_sim_params_row(const grx_sim_params* p, const char* name, float** device_ptr, int* count) {
  if (!p || !name || !device_ptr || !count) return fail("grx_sim_params_row: null argument");
  const int t = grx_param_id(name);
  if (t < 0 || !p->named[t]) return fail(std::string("grx_sim_params_row: '") + name + "' is not a parameter of this object");
  *device_ptr = p->d_stage + p->stage_off[t]; *count = p->cnt[t];
  return 0;
}

extern "C" int grx_sim_params_commit(grx_sim_params* p, const unsigned char* mask, int* invalid, void* stream) {
  if (!p) return fail("grx_sim_params_commit: null object");
  GrxParamCommit a = p->args;
  a.mask = mask; a.bits_out = invalid;
  const int e = grx_tu_simprm_commit(&a, stream);
  if (e) return fail(std::string("grx_sim_params_commit launch: ") + hipGetErrorString((hipError_t)e));
  return 0;
}

extern "C" int grx_sim_step_params(const grx_model* m, const grx_sim_params* p, const grx_sim_buffers* buf, const grx_sim_dynamics* dyn, int n_worlds, int nstep, int forward_only, void* stream) {
  if (!m) return fail("grx_sim_step_params: null model");
  if (!p) return fail("grx_sim_step_params: null parameter object");
  if (m != p->model && m != p->large) return fail("grx_sim_step_params: the parameter object was not created for this model handle");
  if (n_worlds != p->n) return fail("grx_sim_step_params: n_worlds = " + std::to_string(n_worlds) + ", the parameter object holds " + std::to_string(p->n) + " worlds");
  return grx_sim_step_impl({m, buf, dyn, n_worlds, nstep, forward_only, stream, m == p->model ? p->d_desc : p->d_desc_large});
}

// sizeof(GrxParamCommit) is internal; what the Python side mirrors is the list of names, in id order, and the bit of each rule (host only)
extern "C" int grx_sim_params_names(char* out, int cap) {
  const std::string s = grx_param_name_list();
  if (out && cap > 0) { strncpy(out, s.c_str(), (size_t)cap - 1); out[cap - 1] = 0; }
  return (int)s.size();
}

// host only (no device is touched): the float records that depend on table `name`, for one world whose row of that table is `values` -- (a) rec_fill: by the record-fill
// functions the commit kernel calls, on a zeroed region, reading the edited row beside the unedited packed model; (b) rec_build: by grx_build_records on a packed model
// with the same edit.  The record kinds follow each other in the order dof, mpair, jnt, act, pair (those that depend on the table only).  Returns the number of words
// (0: no record depends on the table), -1 on an error; the records are written when cap_words holds them.
extern "C" int grx_sim_params_records(const int32_t* H, const int32_t* I, const double* F, const char* name, const float* values, int n_values, float* rec_fill, float* rec_build, int cap_words) {
  if (!H || !I || !F || !name || !values) return fail("grx_sim_params_records: null argument");
  const int t = grx_param_id(name);
  if (t < 0) return fail(std::string("grx_sim_params_records: no per-world parameter named '") + name + "'; the parameters are " + grx_param_name_list());
  GrxPackedModel pm;
  grx_pack_model(H, I, F, &pm);
  if (n_values != grx_param_table_count(pm, t)) return fail("grx_sim_params_records: " + std::string(name) + " has " + std::to_string(grx_param_table_count(pm, t)) + " words, not " + std::to_string(n_values));
  const GrxParamCounts counts = grx_param_counts(pm);
  const int kinds = grx_param_record_deps(t);
  int words = 0;
  for (int k = 0; k < GRX_NPR; k++) if ((kinds >> k) & 1) words += counts.n[k] * grx_param_record_words(k);
  if (words == 0 || words > cap_words || !rec_fill || !rec_build) return words;
  GrxPackedModel edited = pm;
  const int ti = grx_find_table(pm, name);
  for (int i = 0; i < n_values; i++) edited.f[edited.off[ti] + i] = values[i];
  grx_build_records(&edited, false);
  GrxModel h = grx_bind_model(pm, pm.f.data(), pm.i.data());
  *grx_param_member(&h, t) = values;
  memset(rec_fill, 0, sizeof(float) * (size_t)words);
  int o = 0;
  for (int k = 0; k < GRX_NPR; k++) {
    if (!((kinds >> k) & 1)) continue;
    const int n = counts.n[k] * grx_param_record_words(k);
    *grx_param_record_member(&h, k) = rec_fill + o;
    for (int e = 0; e < counts.n[k]; e++) grx_fill_record(h, k, e, counts.has_dofprm);
    memcpy(rec_build + o, edited.f.data() + grx_param_record_offset(edited, k), sizeof(float) * (size_t)n);
    o += n;
  }
  return words;
}
