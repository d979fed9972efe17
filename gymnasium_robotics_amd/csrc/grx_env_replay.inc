// grx_env_replay.inc -- on-device HER replay attached to a handle (include/grx_replay.h), included at the end of grx_env.hip.
//
// gymnasium_robotics_amd/her.py (HerReplay, continuous=True) without its host mirrors: the worlds whose row of a step is a reset row are read from the index list the step
// left on the device (grx_env::step_list: a host-known length for the Fetch and the host-bookkeeping maze handles, the device word rcount behind rlist for a maze handle
// with device-side bookkeeping), and "is there anything to sample" is answered by the sampling kernel (grx_her_sample_relabel, grx_capi.h).  Per step: one append kernel,
// one relabel kernel, no copy, nothing read back.

struct grx_replay {
  grx_env* e = nullptr;
  int T = 0, R = 0, n = 0, W = 0, od = 0, gd = 0, ad = 0, OW = 0;
  int64_t capacity = 0, max_batch = 0, head = 0, size = 0;
  uint64_t seed = 0, calls = 0;
  bool track = false;             // keep_final in same-step mode: prev_start / term_t / terminal rows are live
  float *episode = nullptr, *actions = nullptr, *rows = nullptr, *term_rows = nullptr;      // term_rows: the replay's own [N, W] (maze) or the Fetch handle's final_packed
  int *start = nullptr, *prev_start = nullptr, *term_t = nullptr, *valid = nullptr;
  std::vector<void*> allocs;
  int t = 0;                      // absolute index of the newest row
  bool begun = false;
  uint64_t epoch = 0, last_step = 0;      // the handle's reset / set_state count at begin; its step count at the last append (or at begin)
  grx_her_args ha{};
  grx_episodes* episodes = nullptr;      // the store of finished episodes attached to this replay (include/grx_episodes.h, grx_env_episodes.inc), or none
};

namespace {

int episodes_archive(grx_replay* r, void* stream);      // grx_env_episodes.inc

// HerReplay.begin_episode + set_episode_start(-elapsed): row 0 <- the packed rows; episode_start from the device counters (elapsed NULL: the host uploaded it already)
__global__ void __launch_bounds__(256) grx_replay_begin_kernel(const float* __restrict__ packed, float* __restrict__ row0, long long n_row, const long long* __restrict__ elapsed, int n,
                                                               int* __restrict__ start, int* __restrict__ prev_start, int* __restrict__ term_t) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  grx_copy_words(row0, packed, n_row, tid, nth);
  for (long long w = tid; w < n; w += nth) {
    if (elapsed) start[w] = -(int)elapsed[w];
    prev_start[w] = 0;
    term_t[w] = -1;
  }
}

unsigned replay_blocks(long long words) {
  long long b = (words / 4 + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

const float* replay_packed(const grx_env* e) { return e->mz ? e->mz->packed : e->packed; }
const float* replay_action(const grx_env* e) { return e->mz ? e->mz->action : e->action; }

template <class T>
int replay_zalloc(grx_replay* r, T** p, size_t count) {
  void* q = nullptr;
  ENV_HIP(hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 1));
  r->allocs.push_back(q);
  ENV_HIP(hipMemset(q, 0, count * sizeof(T)));
  *p = (T*)q;
  return 0;
}

void replay_free(grx_replay* r) {
  for (void* p : r->allocs) (void)hipFree(p);
  delete r;
}

}  // namespace

extern "C" int grx_replay_create(grx_env* e, const grx_replay_config* cfg, grx_replay** out) {
  if (!out) return fail(GRX_ENV_EINVAL, "grx_replay_create: out is NULL");
  *out = nullptr;
  if (!cfg) return fail(GRX_ENV_EINVAL, "grx_replay_create: NULL config");
  if (cfg->horizon < 1 || cfg->horizon > (1 << 20)) return fail(GRX_ENV_EINVAL, "grx_replay_create: horizon " + std::to_string(cfg->horizon) + " out of range (>= 1)");
  if (cfg->capacity < 1) return fail(GRX_ENV_EINVAL, "grx_replay_create: capacity " + std::to_string(cfg->capacity) + " out of range (>= 1)");
  if (cfg->max_batch > cfg->capacity)
    return fail(GRX_ENV_EINVAL, "grx_replay_create: batch " + std::to_string(cfg->max_batch) + " larger than the replay capacity " + std::to_string(cfg->capacity));
  if (!e) return fail(GRX_ENV_EINVAL, "grx_replay_create: NULL handle");
  if (e->replay) return fail(GRX_ENV_EINVAL, "grx_replay_create: the handle already has a replay attached");
  DeviceGuard g(e->device);
  grx_replay* r = new grx_replay();
  r->e = e;
  r->T = cfg->horizon; r->R = r->T + 1; r->n = e->n; r->W = e->pdim; r->od = e->obs_dim; r->gd = e->mz ? 2 : 3; r->ad = e->mz ? e->mz->nu : 4;
  r->OW = 2 * r->od + 3 * r->gd + r->ad + 2;
  r->capacity = cfg->capacity; r->max_batch = cfg->max_batch > 0 ? cfg->max_batch : cfg->capacity;
  r->seed = cfg->seed;
  r->track = cfg->keep_final != 0 && e->mode == GRX_ENV_SAME_STEP;
  const size_t n = (size_t)r->n;
  int rc = [&]() -> int {
    ENV_TRY(replay_zalloc(r, &r->episode, (size_t)r->R * n * r->W));
    ENV_TRY(replay_zalloc(r, &r->actions, (size_t)r->R * n * r->ad));
    ENV_TRY(replay_zalloc(r, &r->rows, (size_t)r->capacity * r->OW));
    ENV_TRY(replay_zalloc(r, &r->start, n)); ENV_TRY(replay_zalloc(r, &r->prev_start, n)); ENV_TRY(replay_zalloc(r, &r->term_t, n));
    ENV_TRY(replay_zalloc(r, &r->valid, 1));
    ENV_HIP(hipMemset(r->term_t, 0xFF, n * 4));      // -1: no episode has ended yet
    if (r->track) {
      if (e->mz) ENV_TRY(replay_zalloc(r, &r->term_rows, n * r->W));
      else r->term_rows = e->final_packed;
    }
    ENV_HIP(hipDeviceSynchronize());
    return 0;
  }();
  if (rc != 0) { std::string msg = g_err; replay_free(r); g_err = msg; return rc; }
  grx_her_args& a = r->ha;
  std::memset(&a, 0, sizeof a);
  a.rows = r->episode; a.acts = r->actions; a.T = r->T; a.N = r->n; a.W = r->W; a.obs_dim = r->od; a.goal_dim = r->gd; a.act_dim = r->ad;
  if (e->mz) { a.kind = 2; a.p0 = e->mz->d.task.goal_radius; a.sparse = e->mz->d.task.sparse_reward; }
  else { a.kind = 0; a.p0 = e->d.task.distance_threshold; a.sparse = e->d.task.sparse_reward; }
  if (r->track) { a.term_rows = r->term_rows; a.term_t = r->term_t; }
  e->replay = r;
  *out = r;
  return 0;
}

extern "C" int grx_replay_destroy(grx_replay* r) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_destroy: NULL replay");
  if (r->episodes) return fail(GRX_ENV_EINVAL, "grx_replay_destroy: an episode store is attached to the replay: grx_episodes_destroy first");
  DeviceGuard g(r->e->device);
  (void)hipDeviceSynchronize();
  r->e->replay = nullptr;
  replay_free(r);
  return 0;
}

extern "C" int grx_replay_dims(const grx_replay* r, int* row_width, int* obs_dim, int* goal_dim, int* act_dim) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_dims: NULL replay");
  if (row_width) *row_width = r->OW;
  if (obs_dim) *obs_dim = r->od;
  if (goal_dim) *goal_dim = r->gd;
  if (act_dim) *act_dim = r->ad;
  return 0;
}

extern "C" int grx_replay_begin(grx_replay* r, void* stream) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_begin: NULL replay");
  grx_env* e = r->e;
  if (!e->has_reset) return fail(GRX_ENV_EINVAL, "grx_replay_begin: cannot begin before grx_env_reset");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  const long long* elapsed_dev = nullptr;
  if (e->mz && !e->mz->host_book) elapsed_dev = e->mz->elapsed;
  else {      // the host's counters, through the handle's pinned ring (enqueued, not waited for)
    const std::vector<int64_t>& el = e->mz ? e->mz->h_elapsed : e->elapsed;
    std::vector<int32_t> neg((size_t)r->n);
    for (int i = 0; i < r->n; ++i) neg[i] = -(int32_t)el[i];
    ENV_TRY(e->upload(r->start, neg.data(), (size_t)r->n * 4, s));
  }
  const long long n_row = (long long)r->n * r->W;
  hipLaunchKernelGGL(grx_replay_begin_kernel, dim3(replay_blocks(n_row)), dim3(256), 0, s, replay_packed(e), r->episode, n_row, elapsed_dev, r->n, r->start, r->prev_start, r->term_t);
  ENV_HIP(hipGetLastError());
  r->t = 0;
  r->begun = true;
  r->epoch = e->epoch;
  r->last_step = e->steps;
  return 0;
}

extern "C" int grx_replay_append(grx_replay* r, void* stream) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_append: NULL replay");
  grx_env* e = r->e;
  if (!r->begun) return fail(GRX_ENV_EINVAL, "grx_replay_append: append before grx_replay_begin");
  if (e->epoch != r->epoch) return fail(GRX_ENV_EINVAL, "grx_replay_append: grx_env_reset / grx_env_set_state since grx_replay_begin: call grx_replay_begin again");
  if (e->steps == r->last_step) return fail(GRX_ENV_EINVAL, "grx_replay_append: no grx_env_step since the last append (double append)");
  if (e->steps != r->last_step + 1) return fail(GRX_ENV_EINVAL, "grx_replay_append: " + std::to_string(e->steps - r->last_step) + " steps since the last append: every step is appended");
  if (r->t == INT32_MAX - 1) return fail(GRX_ENV_EINVAL, "grx_replay_append: row counter exhausted: call grx_replay_begin");
  DeviceGuard g(e->device);
  if (r->episodes) ENV_TRY(episodes_archive(r, stream));      // before this step's row overwrites the oldest ring row and before its worlds are re-marked
  const int t = r->t + 1, row = t % r->R;
  grx_her_append_args a;      // HerReplay.append in one launch (grx_capi.h grx_her_append): the two row copies, the marks of the listed worlds, the terminal-row scatter
  std::memset(&a, 0, sizeof a);
  a.packed = replay_packed(e); a.action = replay_action(e);
  a.n_row = (long long)r->n * r->W; a.n_act = (long long)r->n * r->ad;
  a.row_dst = r->episode + (size_t)row * a.n_row; a.act_dst = r->actions + (size_t)row * a.n_act;
  a.list = e->step_list; a.count_dev = e->step_list ? e->step_count_dev : nullptr; a.count = e->step_list ? e->step_count : 0; a.n_worlds = r->n; a.t = t;
  a.start = r->start;
  if (r->track) {
    a.prev_start = r->prev_start; a.term_t = r->term_t;
    if (e->mz && a.list) { a.final_rows = e->mz->final_rows; a.term_rows = r->term_rows; }
  }
  a.W = r->W;
  ENV_GRX(grx_her_append(&a, stream));
  r->t = t;
  r->last_step = e->steps;
  return 0;
}

extern "C" int grx_replay_relabel(grx_replay* r, int64_t batch, int k_future, grx_replay_batch* out, void* stream) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_relabel: NULL replay");
  if (batch < 1) return fail(GRX_ENV_EINVAL, "grx_replay_relabel: batch " + std::to_string(batch) + " out of range (>= 1)");
  if (batch > r->capacity) return fail(GRX_ENV_EINVAL, "grx_replay_relabel: batch " + std::to_string(batch) + " larger than the replay capacity " + std::to_string(r->capacity));
  if (batch > r->max_batch) return fail(GRX_ENV_EINVAL, "grx_replay_relabel: batch " + std::to_string(batch) + " larger than max_batch " + std::to_string(r->max_batch));
  if (k_future < 0) return fail(GRX_ENV_EINVAL, "grx_replay_relabel: negative k_future");
  DeviceGuard g(r->e->device);
  if (r->head + batch > r->capacity) r->head = 0;      // every batch contiguous (a ring of whole batches)
  grx_her_args a = r->ha;
  a.out = r->rows + (size_t)r->head * r->OW;
  ENV_GRX(grx_her_sample_relabel(&a, r->start, r->track ? r->prev_start : nullptr, r->t, k_future, r->seed, r->calls, batch,
                                 /* scratch: unused since the draws stay in the workgroup, any non-null pointer */ r->valid, r->valid, stream));
  r->calls += 1;
  if (out) { out->rows = a.out; out->batch = batch; out->offset = r->head; out->valid = r->valid; }
  r->head += batch;
  if (r->head > r->size) r->size = r->head;
  return 0;
}

extern "C" int grx_replay_reseed(grx_replay* r, uint64_t seed) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_reseed: NULL replay");
  r->seed = seed;
  r->calls = 0;
  return 0;
}

extern "C" int grx_replay_ring(const grx_replay* r, const float** rows, int64_t* capacity, int64_t* head, int64_t* size) {
  if (!r) return fail(GRX_ENV_EINVAL, "grx_replay_ring: NULL replay");
  if (rows) *rows = r->rows;
  if (capacity) *capacity = r->capacity;
  if (head) *head = r->head;
  if (size) *size = r->size;
  return 0;
}
