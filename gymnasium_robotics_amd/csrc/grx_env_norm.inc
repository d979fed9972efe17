// grx_env_norm.inc -- the observation / goal normaliser attached to a handle (include/grx_norm.h), included at the end of grx_env.hip behind grx_env_episodes.inc.
//
// gymnasium_robotics_amd/her.py (Normalizer) for a caller that is not Python: a stat block of grx_capi.h (grx_normstat_layout) and a buffer for the actor's input, both
// owned here; every call is one or two launches of libgrx_hip.so's kernels with the handle's dimensions filled in.  Nothing is read back outside get / set_state.

struct grx_norm {
  grx_env* e = nullptr;
  int od = 0, gd = 0, ad = 0, W = 0, OW = 0, D = 0, n = 0;
  double eps = 1e-2;
  float clip = 5.0f;
  int64_t lay[8] = {};
  char* stats = nullptr;
  float* policy = nullptr;
};

namespace {

#pragma pack(push, 1)
struct NormBlobHeader {
  char magic[8];
  uint32_t version;
  int32_t obs_dim, goal_dim;
  uint32_t zero0;
  double eps;
  float clip;
  uint32_t zero1;
};
#pragma pack(pop)
static_assert(sizeof(NormBlobHeader) == 40, "state blob header of grx_norm.h");
const char kNormMagic[8] = {'G', 'R', 'X', 'N', 'O', 'R', 'M', '\0'};
constexpr uint32_t kNormVersion = 1;

size_t norm_sums_bytes(const grx_norm* p) { return 16 * (size_t)p->D + 16; }      // sum | sumsq | count | skipped: contiguous at the start of the stat block

void norm_free(grx_norm* p) {
  if (p->stats) (void)hipFree(p->stats);
  if (p->policy) (void)hipFree(p->policy);
  delete p;
}

}  // namespace

extern "C" int grx_norm_create(grx_env* e, const grx_norm_config* cfg, grx_norm** out) {
  if (!out) return fail(GRX_ENV_EINVAL, "grx_norm_create: out is NULL");
  *out = nullptr;
  if (cfg && !(cfg->eps > 0.0)) return fail(GRX_ENV_EINVAL, "grx_norm_create: eps must be positive");
  if (cfg && !(cfg->clip > 0.0f)) return fail(GRX_ENV_EINVAL, "grx_norm_create: clip must be positive");
  if (!e) return fail(GRX_ENV_EINVAL, "grx_norm_create: NULL handle");
  if (e->norm) return fail(GRX_ENV_EINVAL, "grx_norm_create: the handle already has a normalizer attached");
  DeviceGuard g(e->device);
  grx_norm* p = new grx_norm();
  p->e = e;
  p->n = e->n; p->W = e->pdim; p->od = e->obs_dim; p->gd = e->mz ? 2 : 3; p->ad = e->mz ? e->mz->nu : 4;
  p->OW = 2 * p->od + 3 * p->gd + p->ad + 2;
  p->D = p->od + p->gd;
  if (cfg) { p->eps = cfg->eps; p->clip = cfg->clip; }
  int rc = [&]() -> int {
    ENV_GRX(grx_normstat_layout(p->od, p->gd, p->lay));
    ENV_HIP(hipMalloc((void**)&p->stats, (size_t)p->lay[7]));
    ENV_HIP(hipMemset(p->stats, 0, (size_t)p->lay[7]));
    ENV_HIP(hipMalloc((void**)&p->policy, (size_t)p->n * p->D * sizeof(float)));
    ENV_HIP(hipMemset(p->policy, 0, (size_t)p->n * p->D * sizeof(float)));
    ENV_GRX(grx_normstat_refresh(p->stats, p->od, p->gd, p->eps, nullptr));      // count 0: mean 0, inv_std 1
    ENV_HIP(hipDeviceSynchronize());
    return 0;
  }();
  if (rc != 0) { std::string msg = g_err; norm_free(p); g_err = msg; return rc; }
  e->norm = p;
  *out = p;
  return 0;
}

extern "C" int grx_norm_destroy(grx_norm* p) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_norm_destroy: NULL normalizer");
  DeviceGuard g(p->e->device);
  (void)hipDeviceSynchronize();
  p->e->norm = nullptr;
  norm_free(p);
  return 0;
}

extern "C" int grx_norm_dims(const grx_norm* p, int* row_width, int* obs_dim, int* goal_dim, int* act_dim) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_norm_dims: NULL normalizer");
  if (row_width) *row_width = p->OW;
  if (obs_dim) *obs_dim = p->od;
  if (goal_dim) *goal_dim = p->gd;
  if (act_dim) *act_dim = p->ad;
  return 0;
}

extern "C" int grx_norm_update(grx_norm* p, const float* rows, int64_t batch, const int32_t* valid, void* stream) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_norm_update: NULL normalizer");
  if (!rows) return fail(GRX_ENV_EINVAL, "grx_norm_update: NULL rows");
  if (batch < 1) return fail(GRX_ENV_EINVAL, "grx_norm_update: batch " + std::to_string(batch) + " out of range (>= 1)");
  DeviceGuard g(p->e->device);
  ENV_GRX(grx_normstat_update(p->stats, rows, batch, p->OW, p->od, p->gd, valid, p->eps, stream));
  return 0;
}

extern "C" int grx_norm_apply_batch(grx_norm* p, const float* rows, int64_t batch, float* out, void* stream) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_norm_apply_batch: NULL normalizer");
  if (!rows || !out) return fail(GRX_ENV_EINVAL, "grx_norm_apply_batch: NULL rows or out");
  if (batch < 1) return fail(GRX_ENV_EINVAL, "grx_norm_apply_batch: batch " + std::to_string(batch) + " out of range (>= 1)");
  DeviceGuard g(p->e->device);
  ENV_GRX(grx_normstat_apply_batch(p->stats, rows, batch, p->OW, p->od, p->gd, p->ad, p->clip, out, stream));
  return 0;
}

extern "C" int grx_norm_policy_input(grx_norm* p, const float** out, void* stream) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_norm_policy_input: NULL normalizer");
  if (!out) return fail(GRX_ENV_EINVAL, "grx_norm_policy_input: out is NULL");
  if (!p->e->has_reset) return fail(GRX_ENV_EINVAL, "grx_norm_policy_input: the handle has no rows before grx_env_reset");
  DeviceGuard g(p->e->device);
  ENV_GRX(grx_normstat_apply_packed(p->stats, replay_packed(p->e), p->n, p->W, p->od, p->gd, p->clip, p->policy, stream));
  *out = p->policy;
  return 0;
}

extern "C" int grx_norm_stats(const grx_norm* p, const float** mean, const float** inv_std, const double** sum, const double** sumsq, const int64_t** count,
                              const int64_t** skipped, int* dim) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_norm_stats: NULL normalizer");
  if (sum) *sum = (const double*)(p->stats + p->lay[0]);
  if (sumsq) *sumsq = (const double*)(p->stats + p->lay[1]);
  if (count) *count = (const int64_t*)(p->stats + p->lay[2]);
  if (skipped) *skipped = (const int64_t*)(p->stats + p->lay[3]);
  if (mean) *mean = (const float*)(p->stats + p->lay[4]);
  if (inv_std) *inv_std = (const float*)(p->stats + p->lay[5]);
  if (dim) *dim = p->D;
  return 0;
}

extern "C" int grx_norm_state_size(const grx_norm* p, size_t* bytes) {
  if (!p || !bytes) return fail(GRX_ENV_EINVAL, "grx_norm_state_size: NULL argument");
  *bytes = sizeof(NormBlobHeader) + norm_sums_bytes(p);
  return 0;
}

extern "C" int grx_norm_get_state(grx_norm* p, void* blob, size_t bytes) {
  if (!p || !blob) return fail(GRX_ENV_EINVAL, "grx_norm_get_state: NULL argument");
  if (bytes < sizeof(NormBlobHeader) + norm_sums_bytes(p)) return fail(GRX_ENV_EINVAL, "grx_norm_get_state: the buffer is smaller than grx_norm_state_size");
  DeviceGuard g(p->e->device);
  NormBlobHeader h;
  std::memset(&h, 0, sizeof h);
  std::memcpy(h.magic, kNormMagic, 8);
  h.version = kNormVersion; h.obs_dim = p->od; h.goal_dim = p->gd; h.eps = p->eps; h.clip = p->clip;
  std::memcpy(blob, &h, sizeof h);
  ENV_HIP(hipDeviceSynchronize());
  ENV_HIP(hipMemcpy((char*)blob + sizeof h, p->stats, norm_sums_bytes(p), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int grx_norm_set_state(grx_norm* p, const void* blob, size_t bytes) {
  if (!p || !blob) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: NULL argument");
  NormBlobHeader h;
  if (bytes < sizeof h) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: the blob is shorter than its header");
  std::memcpy(&h, blob, sizeof h);
  if (std::memcmp(h.magic, kNormMagic, 8) != 0) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: not a normalizer state blob (bad magic)");
  if (h.version != kNormVersion) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: blob version " + std::to_string(h.version) + ", this library reads version " + std::to_string(kNormVersion));
  if (h.obs_dim != p->od || h.goal_dim != p->gd)
    return fail(GRX_ENV_EINVAL, "grx_norm_set_state: the blob is of dimensions (" + std::to_string(h.obs_dim) + ", " + std::to_string(h.goal_dim) + "), the normalizer of (" +
                                    std::to_string(p->od) + ", " + std::to_string(p->gd) + ")");
  if (bytes != sizeof h + norm_sums_bytes(p)) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: blob of " + std::to_string(bytes) + " bytes, expected " + std::to_string(sizeof h + norm_sums_bytes(p)));
  if (!(h.eps > 0.0) || !(h.clip > 0.0f)) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: the blob's eps and clip must be positive");
  int64_t counts[2];
  std::memcpy(counts, (const char*)blob + sizeof h + 16 * (size_t)p->D, 16);
  if (counts[0] < 0 || counts[1] < 0) return fail(GRX_ENV_EINVAL, "grx_norm_set_state: negative count in the blob");
  DeviceGuard g(p->e->device);
  ENV_HIP(hipDeviceSynchronize());
  ENV_HIP(hipMemcpy(p->stats, (const char*)blob + sizeof h, norm_sums_bytes(p), hipMemcpyHostToDevice));
  p->eps = h.eps; p->clip = h.clip;
  ENV_GRX(grx_normstat_refresh(p->stats, p->od, p->gd, p->eps, nullptr));      // mean / inv_std by the refresh code of update
  ENV_HIP(hipDeviceSynchronize());
  return 0;
}
