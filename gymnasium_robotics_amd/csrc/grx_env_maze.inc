// grx_env_maze.inc -- the maze handle of the env-level C ABI (PointMaze-v3 and AntMaze ids), included by grx_env.hip inside its unnamed namespace.
//
// One step, in every mode of PointMazeVecEnv (envs/point_maze.py: continuing_task, reset_target, the three autoreset modes), all on the caller's stream:
//   actions -> grx_point_step (next-step mode: always the masked launch, its mask is kept on the device) -> grx_maze_episode_end (time limit, termination, update_goal's
//   redraw, the ascending list of worlds to reset and its length, the parked terminal rows) -> grx_maze_sample_resets_list + grx_maze_reset_rows_list over that list ->
//   ONE copy of [terminated | truncated | n_final (| final_idx in same-step mode)] to pinned memory and an event.
// The host decides nothing that depends on the worlds, so nothing here waits for the device; grx_env_outputs waits for the event of that copy only.
//
// Where an episode can only end by the time limit and no goal is redrawn (continuing_task on, reset_target off or a single goal cell: the default mode of every id) the
// host knows every flag and every list in advance, as it does for Fetch: there the handle keeps the counters on the host (host_book) and issues exactly the launches of
// PointMazeVecEnv.step -- the plain step launch and nothing else on a step without a reset -- with no episode-end kernel and no copy of flags.

struct MazeDesc {
  std::vector<int32_t> H, I;
  std::vector<double> F, qpos0, goal_xy, reset_xy;
  grx_point_task task;
  int32_t dims[8];      // nq, nv, nu, obs_dim, obs_skip, n_goal, n_reset, max_episode_steps
  double consts[8];     // goal_radius, position_noise_range, maze_size_scaling, dt, continuing_task, reset_target, sparse_reward, 0
};
static_assert(sizeof(grx_point_task) == 32, "grx_point_task layout");

struct MazeEnv {
  MazeDesc d;
  int nq = 0, nv = 0, nu = 0, obs_skip = 0, n_goal = 0, n_reset = 0, split = 1;
  bool redraw = false;      // MazeEnv.update_goal is live: reset_target && continuing_task && more than one goal cell
  bool host_book = false;   // episodes end by the time limit only and no goal is redrawn: the counters and flags are kept on the host (see the header of this file)
  std::vector<int64_t> h_elapsed;      // host_book: PointMazeVecEnv._elapsed / _needs_reset
  std::vector<uint8_t> h_needs_reset, h_flags;      // h_flags: the flags block of the last call, laid out as flags_dev
  bool success_parked = false;      // host_book, same-step: the last step reset worlds, step_success holds the step's own success flags
  float *qpos, *qvel, *qacc_ws, *goal, *action, *obs, *achieved, *reward, *packed, *final_rows, *stage, *desired, *qpos0;
  unsigned char *success, *term_step, *mask, *needs_reset, *step_success;
  int *status, *split_state = nullptr, *idx, *rlist, *rcount;
  long long* elapsed;
  uint64_t *rng, *rng_rows;
  double *goal_xy, *reset_xy;
  uint8_t *flags_dev = nullptr, *flags_host = nullptr;      // [terminated N | truncated N | pad | n_final | final_idx N]: device block and its pinned mirror
  size_t flags_bytes = 0, off_nfinal = 0, off_idx = 0;
  std::vector<uint8_t> zeros;                               // the same block after a reset / set_state: no flags, no finished worlds
  hipEvent_t flags_ev = nullptr;
  bool flags_live = false;                                  // the last call was a step: the pinned block (behind flags_ev) holds its flags
  grx_point_buffers bufs{}, bufs_masked{};
  grx_maze_reset_args rargs{}, rargs_list{};
  grx_maze_episode_args eargs{};
};

void maze_free(MazeEnv* m) {
  if (!m) return;
  if (m->flags_ev) (void)hipEventDestroy(m->flags_ev);
  if (m->flags_host) (void)hipHostFree(m->flags_host);
  delete m;
}

bool desc_is_maze(const Container& c, std::string* family) {
  auto it = c.sec.find("family");
  if (it == c.sec.end()) { *family = "fetch"; return false; }
  family->assign((const char*)it->second.first, strnlen((const char*)it->second.first, it->second.second));
  return *family == "maze";
}

int parse_maze_desc(const Container& c, MazeDesc* d) {
  ENV_TRY(take<int32_t>(c, "H", -1, &d->H));
  ENV_TRY(take<int32_t>(c, "I", -1, &d->I));
  ENV_TRY(take<double>(c, "F", -1, &d->F));
  ENV_TRY(take<uint8_t>(c, "task", sizeof(grx_point_task), nullptr, &d->task));
  ENV_TRY(take<int32_t>(c, "dims", sizeof d->dims, nullptr, d->dims));
  ENV_TRY(take<double>(c, "consts", sizeof d->consts, nullptr, d->consts));
  const int nq = d->dims[0], nv = d->dims[1], nu = d->dims[2], obs_dim = d->dims[3], skip = d->dims[4], ng = d->dims[5], nr = d->dims[6];
  if (nq < 2 || nv <= 0 || nu <= 0 || (skip != 0 && skip != 2) || obs_dim != nq + nv - skip || ng < 1 || nr < 1 || ng > (1 << 20) || nr > (1 << 20) ||
      (d->task.agent != 0) != (skip == 2) || d->task.n_substeps < 1)
    return fail(GRX_ENV_EDESC, "environment description: inconsistent sizes: dims (nq " + std::to_string(nq) + ", nv " + std::to_string(nv) + ", nu " + std::to_string(nu) + ", obs_dim " +
                                   std::to_string(obs_dim) + ", obs_skip " + std::to_string(skip) + ", " + std::to_string(ng) + " goal / " + std::to_string(nr) +
                                   " reset cells) disagree with each other or with the task struct (agent " + std::to_string(d->task.agent) + ")");
  if ((d->task.continuing_task != 0) != (d->consts[4] != 0.0) || (d->task.sparse_reward != 0) != (d->consts[6] != 0.0) || d->task.goal_radius != d->consts[0])
    return fail(GRX_ENV_EDESC, "environment description: inconsistent sizes: consts (goal radius, continuing_task, sparse reward) disagree with the task struct");
  ENV_TRY(take<double>(c, "qpos0", (int64_t)nq * 8, &d->qpos0));
  ENV_TRY(take<double>(c, "goal_xy", (int64_t)ng * 16, &d->goal_xy));
  ENV_TRY(take<double>(c, "reset_xy", (int64_t)nr * 16, &d->reset_xy));
  return 0;
}

// ------------------------------------------------------------------ the kernels (one thread per listed world)
// rng[idx[j]] <- rows[j] (five uint64 words: a world's new PCG64 stream and its empty 32-bit buffer)
__global__ void __launch_bounds__(64) grx_env_maze_seed_kernel(unsigned long long* __restrict__ rng, const unsigned long long* __restrict__ rows, const int* __restrict__ idx, int k) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  for (int c = 0; c < 5; ++c) rng[(size_t)idx[j] * 5 + c] = rows[(size_t)j * 5 + c];
}

// PointMazeVecEnv._reset_worlds: a reset world starts its episode at step 0, owes no reset and takes part in the next masked step
__global__ void __launch_bounds__(64) grx_env_maze_clear_kernel(long long* __restrict__ elapsed, unsigned char* __restrict__ needs_reset, unsigned char* __restrict__ mask,
                                                                const int* __restrict__ idx, int k) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  const int w = idx[j];
  elapsed[w] = 0; needs_reset[w] = 0; mask[w] = 1;
}

int maze_create(grx_env* e, const grx_env_config* cfg) {
  MazeEnv& m = *e->mz;
  const MazeDesc& d = m.d;
  const int n = e->n;
  m.nq = d.dims[0]; m.nv = d.dims[1]; m.nu = d.dims[2]; m.obs_skip = d.dims[4]; m.n_goal = d.dims[5]; m.n_reset = d.dims[6];
  e->obs_dim = d.dims[3];
  e->pdim = e->obs_dim + 6;
  e->mode = cfg ? cfg->autoreset_mode : GRX_ENV_NEXT_STEP;
  e->max_steps = cfg ? (cfg->max_episode_steps > 0 ? cfg->max_episode_steps : 0) : d.dims[7];
  e->seed_offset = cfg ? cfg->seed_offset : 0;
  e->dt = d.consts[3];
  const bool continuing = d.task.continuing_task != 0, reset_target = d.consts[5] != 0.0;
  m.redraw = reset_target && continuing && m.n_goal > 1;
  m.host_book = continuing && !m.redraw;
  ENV_GRX(grx_model_create(d.H.data(), (int)d.H.size(), d.I.data(), (int)d.I.size(), d.F.data(), (int)d.F.size(), e->device, &e->h));
  if (grx_model_dim(e->h, "nq") != m.nq || grx_model_dim(e->h, "nv") != m.nv || grx_model_dim(e->h, "nu") != m.nu)
    return fail(GRX_ENV_EDESC, "environment description: inconsistent sizes: the model tables disagree with dims");
  // the rows of PointMazeVecEnv.__init__
  ENV_TRY(e->zalloc(&m.qpos, (size_t)n * m.nq)); ENV_TRY(e->zalloc(&m.qvel, (size_t)n * m.nv)); ENV_TRY(e->zalloc(&m.qacc_ws, (size_t)n * m.nv));
  ENV_TRY(e->zalloc(&m.goal, (size_t)n * 2)); ENV_TRY(e->zalloc(&m.action, (size_t)n * m.nu)); ENV_TRY(e->zalloc(&m.obs, (size_t)n * e->obs_dim));
  ENV_TRY(e->zalloc(&m.achieved, (size_t)n * 2)); ENV_TRY(e->zalloc(&m.reward, n)); ENV_TRY(e->zalloc(&m.success, n)); ENV_TRY(e->zalloc(&m.term_step, n));
  ENV_TRY(e->zalloc(&m.status, n)); ENV_TRY(e->zalloc(&m.mask, n)); ENV_TRY(e->zalloc(&m.packed, (size_t)n * e->pdim)); ENV_TRY(e->zalloc(&m.final_rows, (size_t)n * e->pdim));
  ENV_HIP(hipMemset(m.mask, 1, n));
  ENV_TRY(e->zalloc(&m.stage, (size_t)n * 4)); ENV_TRY(e->zalloc(&m.desired, (size_t)n * 2)); ENV_TRY(e->zalloc(&m.qpos0, m.nq));
  ENV_TRY(e->zalloc(&m.needs_reset, n)); ENV_TRY(e->zalloc(&m.step_success, n)); ENV_TRY(e->zalloc(&m.idx, n)); ENV_TRY(e->zalloc(&m.rlist, n)); ENV_TRY(e->zalloc(&m.rcount, 1));
  ENV_TRY(e->zalloc(&m.elapsed, n)); ENV_TRY(e->zalloc(&m.rng, (size_t)n * 5)); ENV_TRY(e->zalloc(&m.rng_rows, (size_t)n * 5));
  ENV_TRY(e->zalloc(&m.goal_xy, (size_t)m.n_goal * 2)); ENV_TRY(e->zalloc(&m.reset_xy, (size_t)m.n_reset * 2));
  std::vector<float> q0(d.qpos0.begin(), d.qpos0.end());
  ENV_HIP(hipMemcpy(m.qpos0, q0.data(), q0.size() * 4, hipMemcpyHostToDevice));
  ENV_HIP(hipMemcpy(m.goal_xy, d.goal_xy.data(), d.goal_xy.size() * 8, hipMemcpyHostToDevice));
  ENV_HIP(hipMemcpy(m.reset_xy, d.reset_xy.data(), d.reset_xy.size() * 8, hipMemcpyHostToDevice));
  m.off_nfinal = ((size_t)2 * n + 3) / 4 * 4;
  m.off_idx = m.off_nfinal + 4;
  m.flags_bytes = m.off_idx + (size_t)4 * n;
  ENV_TRY(e->zalloc(&m.flags_dev, m.flags_bytes));
  ENV_HIP(hipHostMalloc((void**)&m.flags_host, m.flags_bytes, hipHostMallocDefault));
  std::memset(m.flags_host, 0, m.flags_bytes);
  m.zeros.assign(m.flags_bytes, 0);
  m.h_flags.assign(m.flags_bytes, 0);
  m.h_elapsed.assign(n, 0);
  m.h_needs_reset.assign(n, 0);
  ENV_HIP(hipEventCreateWithFlags(&m.flags_ev, hipEventDisableTiming));
  grx_point_buffers& b = m.bufs;
  std::memset(&b, 0, sizeof b);
  b.qpos = m.qpos; b.qvel = m.qvel; b.qacc_ws = m.qacc_ws; b.goal = m.goal; b.action = m.action; b.obs = m.obs; b.achieved = m.achieved; b.reward = m.reward;
  b.success = m.success; b.terminated = m.term_step; b.status = m.status; b.packed = m.packed;
  // the split step of PointMazeVecEnv: MAZE_SPLIT_PARTS (5) for more than one round of worlds, clamped to the frame skip, off below 64 worlds
  const int want = n > 3072 ? 5 : 1, cap = d.task.n_substeps < 8 ? d.task.n_substeps : 8;
  m.split = n >= 64 ? (want < cap ? want : cap) : 1;
  if (m.split < 1) m.split = 1;
  if (m.split > 1) {
    ENV_TRY(e->zalloc(&m.split_state, (size_t)n * 2));
    b.split_state = m.split_state; b.split_parts = m.split;
  }
  m.bufs_masked = b;
  m.bufs_masked.mask = m.mask;
  grx_maze_reset_args& r = m.rargs;
  std::memset(&r, 0, sizeof r);
  r.idx = m.idx; r.stage = m.stage; r.qpos0 = m.qpos0; r.nq = m.nq; r.nv = m.nv; r.obs_dim = e->obs_dim; r.obs_skip = m.obs_skip; r.goal_radius = d.task.goal_radius;
  r.qpos = m.qpos; r.qvel = m.qvel; r.qacc_ws = m.qacc_ws; r.goal = m.goal; r.obs = m.obs; r.achieved = m.achieved; r.reward = m.reward; r.success = m.success; r.packed = m.packed;
  m.rargs_list = r;
  m.rargs_list.idx = m.rlist;
  m.rargs_list.keep_outcome = e->mode == GRX_ENV_SAME_STEP ? 1 : 0;
  grx_maze_episode_args& a = m.eargs;
  std::memset(&a, 0, sizeof a);
  a.elapsed = m.elapsed; a.needs_reset = m.needs_reset; a.success = m.success; a.achieved = m.achieved; a.goal = m.goal; a.status = m.status; a.packed = m.packed; a.rng = m.rng;
  a.goal_xy = m.goal_xy; a.n_goal = m.n_goal; a.mode = e->mode; a.limit = e->max_steps; a.continuing_task = continuing ? 1 : 0; a.reset_target = reset_target ? 1 : 0;
  a.packed_dim = e->pdim; a.noise_range = d.consts[1]; a.scaling = d.consts[2]; a.goal_radius = d.task.goal_radius;
  a.terminated = m.flags_dev; a.truncated = m.flags_dev + n; a.mask = e->mode == GRX_ENV_NEXT_STEP ? m.mask : nullptr;
  a.step_success = e->mode == GRX_ENV_SAME_STEP ? m.step_success : nullptr; a.desired = m.redraw ? m.desired : nullptr;
  a.reset_count = m.rcount; a.reset_idx = m.rlist; a.n_final = (int*)(m.flags_dev + m.off_nfinal); a.final_idx = (int*)(m.flags_dev + m.off_idx);
  a.final_rows = e->mode == GRX_ENV_SAME_STEP ? m.final_rows : nullptr;
  e->pin_bytes = (size_t)n * 40;      // an index list (int32 [N]) or a block of stream rows (uint64 [N, 5])
  for (int s = 0; s < kPinSlots; ++s) {
    ENV_HIP(hipHostMalloc(&e->pin[s], e->pin_bytes, hipHostMallocDefault));
    ENV_HIP(hipEventCreateWithFlags(&e->pin_ev[s], hipEventDisableTiming));
  }
  std::vector<uint64_t> st((size_t)n * 5, 0);      // every world: SeedSequence(None), nothing buffered
  for (int i = 0; i < n; ++i) ENV_TRY(pcg64_from_os(&st[(size_t)i * 5]));
  ENV_HIP(hipMemcpy(m.rng, st.data(), st.size() * 8, hipMemcpyHostToDevice));
  ENV_HIP(hipDeviceSynchronize());
  return 0;
}

int maze_reset(grx_env* e, const uint8_t* mask, const uint64_t* seeds, hipStream_t s) {
  MazeEnv& m = *e->mz;
  auto& L = e->list;
  L.clear();
  for (int i = 0; i < e->n; ++i)
    if (!mask || mask[i]) L.push_back(i);
  const int k = (int)L.size();
  if (k == 0) { m.flags_live = false; m.success_parked = false; e->has_reset = 1; return 0; }
  ENV_TRY(e->upload(m.idx, L.data(), (size_t)k * 4, s));
  if (seeds) {      // the listed worlds' streams: PCG64(SeedSequence(seeds[i])), has_uint32 = 0
    std::vector<uint64_t> rows((size_t)k * 5, 0);
    for (int j = 0; j < k; ++j) pcg64_from_seed(seeds[L[j]], &rows[(size_t)j * 5]);
    ENV_TRY(e->upload(m.rng_rows, rows.data(), rows.size() * 8, s));
    hipLaunchKernelGGL(grx_env_maze_seed_kernel, dim3(blocks(k)), dim3(64), 0, s, (unsigned long long*)m.rng, (const unsigned long long*)m.rng_rows, (const int*)m.idx, k);
    ENV_HIP(hipGetLastError());
  }
  ENV_GRX(grx_maze_sample_resets_device(m.rng, m.idx, k, m.goal_xy, m.n_goal, m.reset_xy, m.n_reset, m.d.consts[1], m.d.consts[2], nullptr, nullptr, m.stage, s));
  ENV_GRX(grx_maze_reset_rows(&m.rargs, k, s));
  hipLaunchKernelGGL(grx_env_maze_clear_kernel, dim3(blocks(k)), dim3(64), 0, s, m.elapsed, m.needs_reset, m.mask, (const int*)m.idx, k);
  ENV_HIP(hipGetLastError());
  if (m.redraw) ENV_HIP(hipMemcpyAsync(m.desired, m.goal, (size_t)e->n * 8, hipMemcpyDeviceToDevice, s));
  for (int w : L) { m.h_elapsed[w] = 0; m.h_needs_reset[w] = 0; }
  m.flags_live = false;
  m.success_parked = false;
  e->has_reset = 1;
  return 0;
}

// host_book: PointMazeVecEnv.step as it stands (envs/point_maze.py), the host deciding the time limit -- no world can end otherwise in these modes
int maze_step_host_book(grx_env* e, hipStream_t s) {
  MazeEnv& m = *e->mz;
  const int n = e->n;
  auto& pending = e->list;
  pending.clear();
  if (e->mode == GRX_ENV_NEXT_STEP)
    for (int i = 0; i < n; ++i)
      if (m.h_needs_reset[i]) pending.push_back(i);
  const int kp = (int)pending.size();
  if (kp) {
    ENV_TRY(e->upload(m.idx, pending.data(), (size_t)kp * 4, s));
    ENV_HIP(hipMemsetAsync(m.mask, 1, n, s));
    hipLaunchKernelGGL(grx_env_mask_kernel, dim3(blocks(kp)), dim3(64), 0, s, m.mask, (const int*)m.idx, kp);
    ENV_HIP(hipGetLastError());
  }
  ENV_GRX(grx_point_step(e->h, &m.d.task, kp ? &m.bufs_masked : &m.bufs, n, s));
  uint8_t* f = m.h_flags.data();
  int32_t* fidx = (int32_t*)(f + m.off_idx);
  auto& done = e->will;
  done.clear();
  for (int i = 0; i < n; ++i) {
    const bool stepped = !m.h_needs_reset[i];
    if (stepped) m.h_elapsed[i] += 1;
    const bool trunc = stepped && e->max_steps > 0 && m.h_elapsed[i] >= e->max_steps;
    f[i] = 0; f[n + i] = trunc ? 1 : 0;
    if (trunc) done.push_back(i);
  }
  int n_final = 0;
  m.success_parked = false;
  if (kp) {      // next-step autoreset: the reset replaces the step of the pending worlds
    ENV_GRX(grx_maze_sample_resets_device(m.rng, m.idx, kp, m.goal_xy, m.n_goal, m.reset_xy, m.n_reset, m.d.consts[1], m.d.consts[2], nullptr, nullptr, m.stage, s));
    m.rargs.keep_outcome = 0;
    ENV_GRX(grx_maze_reset_rows(&m.rargs, kp, s));
    for (int w : pending) { m.h_elapsed[w] = 0; m.h_needs_reset[w] = 0; }
    e->step_list = m.idx; e->step_count = kp;
  }
  const int kd = (int)done.size();
  if (e->mode == GRX_ENV_NEXT_STEP) {
    for (int w : done) m.h_needs_reset[w] = 1;
  } else if (e->mode == GRX_ENV_SAME_STEP && kd) {      // the terminal rows and the step's own success flags are parked before the reset overwrites them
    ENV_TRY(e->upload(m.idx, done.data(), (size_t)kd * 4, s));
    hipLaunchKernelGGL(grx_env_gather_kernel, dim3(blocks(kd)), dim3(64), 0, s, m.final_rows, (const float*)m.packed, e->pdim, (const int*)m.idx, kd);
    ENV_HIP(hipGetLastError());
    ENV_HIP(hipMemcpyAsync(m.step_success, m.success, n, hipMemcpyDeviceToDevice, s));
    ENV_GRX(grx_maze_sample_resets_device(m.rng, m.idx, kd, m.goal_xy, m.n_goal, m.reset_xy, m.n_reset, m.d.consts[1], m.d.consts[2], nullptr, nullptr, m.stage, s));
    m.rargs.keep_outcome = 1;
    ENV_GRX(grx_maze_reset_rows(&m.rargs, kd, s));
    m.rargs.keep_outcome = 0;
    for (int j = 0; j < kd; ++j) { fidx[j] = done[j]; m.h_elapsed[done[j]] = 0; }
    n_final = kd;
    m.success_parked = true;
    e->step_list = m.idx; e->step_count = kd;
  }
  std::memcpy(f + m.off_nfinal, &n_final, 4);
  m.flags_live = true;
  return 0;
}

int maze_step(grx_env* e, const float* actions, hipStream_t s) {
  MazeEnv& m = *e->mz;
  const int n = e->n;
  ENV_HIP(hipMemcpyAsync(m.action, actions, (size_t)n * m.nu * 4, hipMemcpyDefault, s));
  if (m.host_book) return maze_step_host_book(e, s);
  ENV_GRX(grx_point_step(e->h, &m.d.task, e->mode == GRX_ENV_NEXT_STEP ? &m.bufs_masked : &m.bufs, n, s));
  ENV_GRX(grx_maze_episode_end(&m.eargs, n, s));
  e->step_list = m.rlist; e->step_count_dev = m.rcount;      // (the list and its length stay on the device: an attached replay reads them there)
  if (e->mode != GRX_ENV_DISABLED) {
    ENV_GRX(grx_maze_sample_resets_list(m.rng, m.rlist, m.rcount, n, m.goal_xy, m.n_goal, m.reset_xy, m.n_reset, m.d.consts[1], m.d.consts[2], m.stage, s));
    ENV_GRX(grx_maze_reset_rows_list(&m.rargs_list, m.rcount, n, m.redraw ? m.desired : nullptr, s));
  }
  // (final_idx is written in same-step mode only: the other modes copy the flags and the zero count)
  ENV_HIP(hipMemcpyAsync(m.flags_host, m.flags_dev, e->mode == GRX_ENV_SAME_STEP ? m.flags_bytes : m.off_idx, hipMemcpyDeviceToHost, s));
  ENV_HIP(hipEventRecord(m.flags_ev, s));
  m.flags_live = true;
  return 0;
}

// the host block of the last call, waiting for its copy only (not for the device)
int maze_flags(const grx_env* e, const uint8_t** f) {
  const MazeEnv& m = *e->mz;
  if (m.host_book) { *f = m.flags_live ? m.h_flags.data() : m.zeros.data(); return 0; }
  if (m.flags_live) ENV_HIP(hipEventSynchronize(m.flags_ev));
  *f = m.flags_live ? m.flags_host : m.zeros.data();
  return 0;
}

int maze_outputs(const grx_env* e, grx_env_device_outputs* out) {
  const MazeEnv& m = *e->mz;
  const uint8_t* f = nullptr;
  ENV_TRY(maze_flags(e, &f));
  out->num_envs = e->n; out->obs_dim = e->obs_dim; out->goal_dim = 2; out->packed_dim = e->pdim;
  out->obs = m.obs; out->achieved = m.achieved; out->desired = m.redraw ? m.desired : m.goal; out->reward = m.reward;
  out->success = (m.host_book ? m.success_parked : m.flags_live && e->mode == GRX_ENV_SAME_STEP) ? m.step_success : m.success;
  out->status = m.status; out->packed = m.packed;
  out->terminated = f; out->truncated = f + e->n;
  std::memcpy(&out->n_final, f + m.off_nfinal, 4);
  out->final_idx = (const int32_t*)(f + m.off_idx); out->final_rows = m.final_rows;
  return 0;
}

int maze_copy_outputs(grx_env* e, grx_env_host_outputs* out) {
  grx_env_device_outputs o;
  ENV_HIP(hipDeviceSynchronize());
  ENV_TRY(maze_outputs(e, &o));
  const size_t n = e->n;
  auto d2h = [](void* dst, const void* src, size_t bytes) { return (dst && bytes) ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
  ENV_HIP(d2h(out->obs, o.obs, n * e->obs_dim * 4));
  ENV_HIP(d2h(out->achieved, o.achieved, n * 8));
  ENV_HIP(d2h(out->desired, o.desired, n * 8));
  ENV_HIP(d2h(out->reward, o.reward, n * 4));
  ENV_HIP(d2h(out->success, o.success, n));
  ENV_HIP(d2h(out->status, o.status, n * 4));
  ENV_HIP(d2h(out->packed, o.packed, n * e->pdim * 4));
  ENV_HIP(d2h(out->final_rows, o.final_rows, (size_t)o.n_final * e->pdim * 4));
  if (out->terminated) std::memcpy(out->terminated, o.terminated, n);
  if (out->truncated) std::memcpy(out->truncated, o.truncated, n);
  if (out->n_final) *out->n_final = o.n_final;
  if (out->final_idx && o.n_final) std::memcpy(out->final_idx, o.final_idx, (size_t)o.n_final * 4);
  return 0;
}
