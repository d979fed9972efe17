// grx_env_episodes.inc -- the store of finished episodes attached to a replay (include/grx_episodes.h), included at the end of grx_env.hip behind grx_env_replay.inc.
//
// gymnasium_robotics_amd/her.py (EpisodicHerReplay) without its host mirrors: grx_replay_append calls episodes_archive before its own launch, which hands the list the step
// left on the device (grx_env::step_list / step_count / step_count_dev) to grx_her_archive; grx_episodes_sample is one launch of grx_her_episode_sample (grx_capi.h).
// Nothing is copied and nothing is read back.

struct grx_episodes {
  grx_replay* r = nullptr;
  int64_t E = 0, max_batch = 0;
  uint64_t seed = 0, calls = 0;
  float *rows = nullptr, *acts = nullptr, *out = nullptr;
  int *meta = nullptr, *valid = nullptr;
  long long* count = nullptr;
  std::vector<void*> allocs;
};

namespace {

template <class T>
int episodes_zalloc(grx_episodes* p, T** q, size_t count) {
  void* m = nullptr;
  ENV_HIP(hipMalloc(&m, count * sizeof(T) > 0 ? count * sizeof(T) : 1));
  p->allocs.push_back(m);
  ENV_HIP(hipMemset(m, 0, count * sizeof(T)));
  *q = (T*)m;
  return 0;
}

void episodes_free(grx_episodes* p) {
  for (void* m : p->allocs) (void)hipFree(m);
  delete p;
}

// the episodes that ended in the step about to be appended -> the store; r->t is still the index of the newest ring row, r->start still holds the marks of those episodes
int episodes_archive(grx_replay* r, void* stream) {
  grx_env* e = r->e;
  grx_episodes* p = r->episodes;
  if (!e->step_list || (!e->step_count_dev && e->step_count <= 0)) return 0;      // host-known: the step ended no episode
  grx_her_archive_args a;
  std::memset(&a, 0, sizeof a);
  a.rows = r->episode; a.acts = r->actions; a.start = r->start;
  a.list = e->step_list; a.count_dev = e->step_count_dev; a.count = e->step_count;
  a.n_worlds = r->n; a.T = r->T; a.W = r->W; a.act_dim = r->ad; a.t_prev = r->t;
  if (r->track) {      // the terminal rows of this step: per world (Fetch) or in list order (maze), and the actions that led to them
    a.final_rows = e->mz ? e->mz->final_rows : e->final_packed;
    a.final_compact = e->mz ? 1 : 0;
    a.step_action = replay_action(e);
  }
  a.ep_rows = p->rows; a.ep_acts = p->acts; a.ep_meta = p->meta; a.ep_count = p->count; a.episodes = p->E;
  ENV_GRX(grx_her_archive(&a, stream));
  return 0;
}

}  // namespace

extern "C" int grx_episodes_create(grx_replay* r, const grx_episodes_config* cfg, grx_episodes** out) {
  if (!out) return fail(GRX_ENV_EINVAL, "grx_episodes_create: out is NULL");
  *out = nullptr;
  if (!cfg) return fail(GRX_ENV_EINVAL, "grx_episodes_create: NULL config");
  if (cfg->max_batch < 1) return fail(GRX_ENV_EINVAL, "grx_episodes_create: max_batch " + std::to_string(cfg->max_batch) + " out of range (>= 1)");
  if (cfg->episodes >= (1ll << 31)) return fail(GRX_ENV_EINVAL, "grx_episodes_create: episodes " + std::to_string(cfg->episodes) + " out of range (< 2^31)");
  if (!r) return fail(GRX_ENV_EINVAL, "grx_episodes_create: NULL replay");
  if (cfg->episodes < r->n)
    return fail(GRX_ENV_EINVAL, "grx_episodes_create: episodes " + std::to_string(cfg->episodes) + " is less than the number of worlds " + std::to_string(r->n));
  if (r->episodes) return fail(GRX_ENV_EINVAL, "grx_episodes_create: the replay already has a store attached");
  DeviceGuard g(r->e->device);
  grx_episodes* p = new grx_episodes();
  p->r = r; p->E = cfg->episodes; p->max_batch = cfg->max_batch; p->seed = cfg->seed;
  const size_t E = (size_t)p->E, R = (size_t)r->R;
  int rc = [&]() -> int {
    ENV_TRY(episodes_zalloc(p, &p->rows, E * R * r->W));
    ENV_TRY(episodes_zalloc(p, &p->acts, E * R * r->ad));
    ENV_TRY(episodes_zalloc(p, &p->meta, E * 4));
    ENV_TRY(episodes_zalloc(p, &p->count, 1));
    ENV_TRY(episodes_zalloc(p, &p->out, (size_t)p->max_batch * r->OW));
    ENV_TRY(episodes_zalloc(p, &p->valid, 1));
    ENV_HIP(hipDeviceSynchronize());
    return 0;
  }();
  if (rc != 0) { std::string msg = g_err; episodes_free(p); g_err = msg; return rc; }
  r->episodes = p;
  *out = p;
  return 0;
}

extern "C" int grx_episodes_destroy(grx_episodes* p) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_episodes_destroy: NULL store");
  DeviceGuard g(p->r->e->device);
  (void)hipDeviceSynchronize();
  p->r->episodes = nullptr;
  episodes_free(p);
  return 0;
}

extern "C" int grx_episodes_dims(const grx_episodes* p, int* row_width, int* horizon, int* packed_width, int* act_dim) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_episodes_dims: NULL store");
  if (row_width) *row_width = p->r->OW;
  if (horizon) *horizon = p->r->T;
  if (packed_width) *packed_width = p->r->W;
  if (act_dim) *act_dim = p->r->ad;
  return 0;
}

extern "C" int grx_episodes_sample(grx_episodes* p, int64_t batch, int k_future, int strategy, grx_episodes_batch* out, void* stream) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_episodes_sample: NULL store");
  if (batch < 1) return fail(GRX_ENV_EINVAL, "grx_episodes_sample: batch " + std::to_string(batch) + " out of range (>= 1)");
  if (batch > p->max_batch) return fail(GRX_ENV_EINVAL, "grx_episodes_sample: batch " + std::to_string(batch) + " larger than max_batch " + std::to_string(p->max_batch));
  if (k_future < 0) return fail(GRX_ENV_EINVAL, "grx_episodes_sample: negative k_future");
  if (strategy != GRX_EPISODES_FUTURE && strategy != GRX_EPISODES_FINAL && strategy != GRX_EPISODES_EPISODE)
    return fail(GRX_ENV_EINVAL, "grx_episodes_sample: unknown strategy " + std::to_string(strategy));
  DeviceGuard g(p->r->e->device);
  ENV_GRX(grx_her_episode_sample(&p->r->ha, p->rows, p->acts, p->meta, p->count, p->E, strategy, k_future, p->seed, p->calls, batch, p->out, p->valid, stream));
  p->calls += 1;
  if (out) { out->rows = p->out; out->batch = batch; out->valid = p->valid; }
  return 0;
}

extern "C" int grx_episodes_reseed(grx_episodes* p, uint64_t seed) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_episodes_reseed: NULL store");
  p->seed = seed;
  p->calls = 0;
  return 0;
}

extern "C" int grx_episodes_store(const grx_episodes* p, const float** rows, const float** acts, const int32_t** meta, const int64_t** count_dev, int64_t* episodes) {
  if (!p) return fail(GRX_ENV_EINVAL, "grx_episodes_store: NULL store");
  if (rows) *rows = p->rows;
  if (acts) *acts = p->acts;
  if (meta) *meta = p->meta;
  if (count_dev) *count_dev = (const int64_t*)p->count;
  if (episodes) *episodes = p->E;
  return 0;
}
