// grx_env.hip -- env-level C ABI (include/grx_env.h).  Two handle kinds behind the same entry points: the Fetch family below -- the launch group of
// FetchVecEnv(output="torch").step (envs/fetch.py) in C++, on top of libgrx_hip.so's entry points, plus the few small kernels that replace the torch operations of that
// step -- and the maze family (PointMaze / AntMaze) in grx_env_maze.inc, whose episode bookkeeping runs on the device.
//
// One step, as envs/fetch.py issues it by default:
//   next-step resets pending:  mask <- 1, 0 for the pending worlds (grx_env_mask_kernel); the masked step launch
//   else:                      the plain step launch
//   every step launch:         split parts (FETCH_SPLIT_PARTS / FETCH_SPLIT_WIDE), hull caches, cost-ordered dispatch; then the entry-mode overflow re-run on the
//                              large tables (core.OverflowLane.rerun_only) and grx_order_by_cost_slots
//   same-step autoreset:       the worlds the step truncates are known before it: their reset (draws + grx_fetch_reset into staged rows) runs on the side stream
//                              behind the step launch ("after" order), grx_fetch_commit_rows behind the step commits it, grx_env_gather_kernel copies the parked
//                              terminal rows out
//   next-step autoreset:       the pending worlds are reset behind the masked step; reward / packed reward zeroed (grx_env_zero_outcome_kernel)
// Host bookkeeping (time limit, flags) as in FetchVecEnv.step.  Index lists reach the device through a ring of pinned buffers; the host never waits for the device in
// grx_env_step.
//
// An on-device HER replay can be attached to a handle of either kind (include/grx_replay.h, grx_env_replay.inc): every step leaves behind, in host fields only, where the
// list of the worlds it reset lives on the device (step_list / step_count / step_count_dev).  A handle without a replay issues the same launches either way.
#include <hip/hip_runtime.h>

#include <sys/random.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "grx_capi.h"
#include "grx_env.h"
#include "grx_replay.h"
#include "grx_episodes.h"
#include "grx_norm.h"
#include "grx_copy.h"

namespace {

constexpr int kEntryCap = 256;          // core.ENTRY_CAP
constexpr int kSplitParts = 4;          // envs/fetch.py FETCH_SPLIT_PARTS
constexpr int kSplitWide = 12288;       // envs/fetch.py FETCH_SPLIT_WIDE
constexpr double kLaneMargin = 0.8;     // core.LANE_MARGIN
constexpr int kLaneTtl = 4;             // core.LANE_TTL
constexpr float kBalanceAlpha = 0.1f;   // FetchVecEnv.balance_alpha
constexpr int kHullWords = 90;          // grx_fetch_buffers.hullcache
constexpr int kPinSlots = 16;           // core.PinnedStager

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define ENV_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(GRX_ENV_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define ENV_GRX(expr) do { if ((expr) != 0) return fail(GRX_ENV_EHIP, std::string(#expr) + ": " + grx_last_error()); } while (0)
#define ENV_TRY(expr) do { int r_ = (expr); if (r_ != 0) return r_; } while (0)

// ------------------------------------------------------------------ the kernels (one thread per listed world, wave64, no atomics)
// mask[idx[j]] <- 0 (behind a fill of ones): the worlds of a next-step reset sit out the masked step launch
__global__ void __launch_bounds__(64) grx_env_mask_kernel(unsigned char* __restrict__ mask, const int* __restrict__ idx, int k) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j < k) mask[idx[j]] = 0;
}

// next-step autoreset: the reset replaces the step, reward 0 (reward[w] and the reward word of the packed row)
__global__ void __launch_bounds__(64) grx_env_zero_outcome_kernel(float* __restrict__ reward, float* __restrict__ packed, int pdim, const int* __restrict__ idx, int k) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  const int w = idx[j];
  reward[w] = 0.0f;
  packed[(size_t)w * pdim + pdim - 2] = 0.0f;
}

// rows[j] <- src[idx[j]] (final_rows from final_packed; width words per row)
__global__ void __launch_bounds__(64) grx_env_gather_kernel(float* __restrict__ rows, const float* __restrict__ src, int width, const int* __restrict__ idx, int k) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  const float* s = src + (size_t)idx[j] * width;
  float* d = rows + (size_t)j * width;
  for (int c = 0; c < width; ++c) d[c] = s[c];
}

// rng[idx[j]] <- rows[j] (four uint64 words: a world's new PCG64 stream)
__global__ void __launch_bounds__(64) grx_env_scatter_rng_kernel(unsigned long long* __restrict__ rng, const unsigned long long* __restrict__ rows, const int* __restrict__ idx, int k) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  for (int c = 0; c < 4; ++c) rng[(size_t)idx[j] * 4 + c] = rows[(size_t)j * 4 + c];
}

unsigned blocks(int k) { return (unsigned)((k + 63) / 64); }

// ------------------------------------------------------------------ numpy SeedSequence -> PCG64 (numpy/random/bit_generator.pyx, pcg64.pyx)
void pcg64_from_entropy(const std::vector<uint32_t>& ent, uint64_t out[4]) {
  const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu, MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
  uint32_t hc = INIT_A, pool[4];
  auto hashmix = [&hc, MULT_A](uint32_t v) { v ^= hc; hc *= MULT_A; v *= hc; v ^= v >> 16; return v; };
  auto mix = [MIX_L, MIX_R](uint32_t x, uint32_t y) { uint32_t r = MIX_L * x - MIX_R * y; r ^= r >> 16; return r; };
  const size_t m = ent.size();
  for (size_t i = 0; i < 4; ++i) pool[i] = hashmix(i < m ? ent[i] : 0u);
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 4; ++d)
      if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
  for (size_t s = 4; s < m; ++s)
    for (int d = 0; d < 4; ++d) pool[d] = mix(pool[d], hashmix(ent[s]));
  uint32_t st[8], hb = INIT_B;      // generate_state(4, np.uint64)
  for (int i = 0; i < 8; ++i) {
    uint32_t v = pool[i % 4];
    v ^= hb; hb *= MULT_B; v *= hb; v ^= v >> 16;
    st[i] = v;
  }
  uint64_t val[4];
  for (int j = 0; j < 4; ++j) val[j] = (uint64_t)st[2 * j] | ((uint64_t)st[2 * j + 1] << 32);
  typedef unsigned __int128 u128;
  const u128 M = ((u128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull;     // PCG_DEFAULT_MULTIPLIER_128
  const u128 initstate = ((u128)val[0] << 64) | val[1], initseq = ((u128)val[2] << 64) | val[3];
  const u128 inc = (initseq << 1) | 1u;     // pcg_setseq_128_srandom_r
  u128 state = inc;                         // 0 * M + inc
  state += initstate;
  state = state * M + inc;
  out[0] = (uint64_t)(state >> 64); out[1] = (uint64_t)state; out[2] = (uint64_t)(inc >> 64); out[3] = (uint64_t)inc;
}

void pcg64_from_seed(uint64_t seed, uint64_t out[4]) {
  std::vector<uint32_t> w;      // numpy's int -> uint32 words, least significant first, no leading zero words (0 -> [0])
  do { w.push_back((uint32_t)seed); seed >>= 32; } while (seed);
  pcg64_from_entropy(w, out);
}

int pcg64_from_os(uint64_t out[4]) {      // SeedSequence(None): 128 bits of OS entropy
  uint32_t r[4];
  size_t got = 0;
  while (got < sizeof r) {
    ssize_t k = getrandom((char*)r + got, sizeof r - got, 0);
    if (k < 0) return fail(GRX_ENV_EINVAL, "getrandom failed: no OS entropy");
    got += (size_t)k;
  }
  std::vector<uint32_t> w(r, r + 4);
  while (w.size() > 1 && w.back() == 0) w.pop_back();
  pcg64_from_entropy(w, out);
  return 0;
}

// ------------------------------------------------------------------ the section container (gymnasium_robotics_amd/env_capi.py)
struct Header { char magic[8]; uint32_t version, n_sections; char env_id[48]; int64_t num_envs; uint64_t total_bytes; };
struct Entry { char name[24]; uint64_t offset, bytes; };
static_assert(sizeof(Header) == 80 && sizeof(Entry) == 40, "container layout");
static_assert(sizeof(grx_fetch_task) == 96, "grx_fetch_task layout");
const char kDescMagic[8] = {'G', 'R', 'X', 'E', 'N', 'V', 'D', 0};
const char kStateMagic[8] = {'G', 'R', 'X', 'E', 'N', 'V', 'S', 0};

struct Container {
  Header h;
  std::map<std::string, std::pair<const uint8_t*, uint64_t>> sec;
};

int parse_container(const uint8_t* p, size_t size, const char* magic, uint32_t version, const char* what, int code, Container* c) {
  if (size < sizeof(Header)) return fail(code, std::string(what) + ": truncated (" + std::to_string(size) + " bytes, the header alone is 80)");
  std::memcpy(&c->h, p, sizeof(Header));
  if (std::memcmp(c->h.magic, magic, 8) != 0) return fail(code, std::string(what) + ": wrong magic (not a " + std::string(magic) + " file)");
  if (c->h.version != version)
    return fail(code, std::string(what) + ": unsupported version " + std::to_string(c->h.version) + " (this library reads version " + std::to_string(version) + ")");
  if (c->h.total_bytes != size) {
    if (size < c->h.total_bytes) return fail(code, std::string(what) + ": truncated (" + std::to_string(size) + " of " + std::to_string(c->h.total_bytes) + " bytes)");
    return fail(code, std::string(what) + ": " + std::to_string(size) + " bytes, the header says " + std::to_string(c->h.total_bytes));
  }
  if (c->h.n_sections > 4096 || sizeof(Header) + (uint64_t)c->h.n_sections * sizeof(Entry) > size)
    return fail(code, std::string(what) + ": truncated section table (" + std::to_string(c->h.n_sections) + " sections)");
  for (uint32_t k = 0; k < c->h.n_sections; ++k) {
    Entry e;
    std::memcpy(&e, p + sizeof(Header) + k * sizeof(Entry), sizeof(Entry));
    e.name[23] = 0;
    if (e.offset > size || e.bytes > size - e.offset) return fail(code, std::string(what) + ": section '" + e.name + "' runs past the end of the data (truncated)");
    c->sec[e.name] = {p + e.offset, e.bytes};
  }
  return 0;
}

struct Desc {
  std::string env_id;
  std::vector<int32_t> H, I, Hr, Ir;
  std::vector<double> F, Fr, q0, mocap0;
  grx_fetch_task task;
  int32_t dims[8];
  double consts[11];
  int32_t caps[3];
};

// copies section `name` into dst; `expect` bytes (or a multiple of `unit` when expect < 0)
template <class T>
int take(const Container& c, const char* name, int64_t expect, std::vector<T>* dst, void* raw = nullptr) {
  auto it = c.sec.find(name);
  if (it == c.sec.end()) return fail(GRX_ENV_EDESC, std::string("environment description: section '") + name + "' is missing");
  const uint64_t b = it->second.second;
  if (expect >= 0 && b != (uint64_t)expect)
    return fail(GRX_ENV_EDESC, std::string("environment description: inconsistent sizes: section '") + name + "' holds " + std::to_string(b) + " bytes, expected " +
                                   std::to_string(expect));
  if (b % sizeof(T) != 0 || (expect < 0 && b == 0))
    return fail(GRX_ENV_EDESC, std::string("environment description: inconsistent sizes: section '") + name + "' holds " + std::to_string(b) + " bytes, not a positive multiple of " +
                                   std::to_string(sizeof(T)));
  if (dst) { dst->resize(b / sizeof(T)); std::memcpy(dst->data(), it->second.first, b); }
  if (raw) std::memcpy(raw, it->second.first, b);
  return 0;
}

// the file into buf and its section table into c (which points into buf)
int read_desc(const char* path, std::vector<uint8_t>* bufp, Container* cp) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(GRX_ENV_EDESC, std::string("environment description: cannot open ") + path);
  std::vector<uint8_t>& buf = *bufp;
  uint8_t chunk[1 << 16];
  size_t k;
  while ((k = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + k);
  std::fclose(f);
  Container& c = *cp;
  ENV_TRY(parse_container(buf.data(), buf.size(), kDescMagic, GRX_ENV_DESC_VERSION, "environment description", GRX_ENV_EDESC, &c));
  c.h.env_id[47] = 0;
  return 0;
}

struct MazeEnv;      // the maze handle (grx_env_maze.inc)
void maze_free(MazeEnv* m);

int parse_desc(const Container& c, Desc* d) {
  ENV_TRY(take<int32_t>(c, "H", -1, &d->H));
  ENV_TRY(take<int32_t>(c, "I", -1, &d->I));
  ENV_TRY(take<double>(c, "F", -1, &d->F));
  ENV_TRY(take<int32_t>(c, "H_rerun", (int64_t)(d->H.size() * 4), &d->Hr));
  ENV_TRY(take<int32_t>(c, "I_rerun", (int64_t)(d->I.size() * 4), &d->Ir));
  ENV_TRY(take<double>(c, "F_rerun", (int64_t)(d->F.size() * 8), &d->Fr));
  ENV_TRY(take<uint8_t>(c, "task", sizeof(grx_fetch_task), nullptr, &d->task));
  ENV_TRY(take<int32_t>(c, "dims", sizeof d->dims, nullptr, d->dims));
  ENV_TRY(take<double>(c, "consts", sizeof d->consts, nullptr, d->consts));
  ENV_TRY(take<int32_t>(c, "fast_caps", sizeof d->caps, nullptr, d->caps));
  const int nq = d->dims[0], nv = d->dims[1], nmocap = d->dims[2], obs_dim = d->dims[4];
  if (nq <= 0 || nv <= 0 || nmocap != 1 || obs_dim != d->task.obs_dim || d->task.goal_dim != 3 || d->dims[5] >= nq)
    return fail(GRX_ENV_EDESC, "environment description: inconsistent sizes: dims (nq " + std::to_string(nq) + ", nv " + std::to_string(nv) + ", nmocap " + std::to_string(nmocap) +
                                   ", obs_dim " + std::to_string(obs_dim) + ") disagree with the task struct (obs_dim " + std::to_string(d->task.obs_dim) + ")");
  ENV_TRY(take<double>(c, "q0", (int64_t)nq * 8, &d->q0));
  ENV_TRY(take<double>(c, "mocap0", (int64_t)nmocap * 56, &d->mocap0));
  return 0;
}

}  // namespace

// ------------------------------------------------------------------ the handle
struct grx_env {
  int device = 0, n = 0, mode = GRX_ENV_NEXT_STEP, max_steps = 0;
  uint64_t seed_offset = 0;
  Desc d;
  MazeEnv* mz = nullptr;      // a maze handle: the fields below the model handle `h` are the Fetch handle's and stay unused
  grx_model *h = nullptr, *hbig = nullptr;
  int nq = 0, nv = 0, nmocap = 0, nu = 0, obs_dim = 0, pdim = 0, obj_qadr = -1;
  double g0[3] = {0, 0, 0}, toff[3] = {0, 0, 0}, height_offset = 0, dt = 0;
  int soft[4] = {0, 0, 0, 0};
  std::vector<void*> allocs;
  // device rows (FetchVecEnv._alloc)
  float *qpos, *qvel, *qacc_ws, *mocap, *aux, *goal, *action, *obs, *achieved, *reward, *packed, *final_packed, *final_rows, *hullcache, *cost_ema = nullptr;
  unsigned char *success, *mask;
  int *status, *cost = nullptr, *order = nullptr;
  float* split_rows = nullptr;
  int* split_state = nullptr;
  uint64_t *rng, *rng_rows;
  float *init_qpos, *init_qvel, *init_mocap;
  int *idx_main, *idx_ahead;
  float *samp_main, *samp_ahead;
  int* lane_head;     // core._LaneBuf: flags [N] u8 | next_count | entry_count
  int *lane_next_list, *lane_entry_list;
  signed char* lane_ttl;
  size_t lane_head_bytes = 0;
  float *a_qpos, *a_qvel, *a_qacc_ws, *a_mocap, *a_aux, *a_goal, *a_obs, *a_achieved, *a_reward;
  unsigned char* a_success;
  int* a_status;
  grx_fetch_buffers bufs{}, bufs_masked{}, lane_plain{}, lane_masked{}, ahead_bufs{};
  bool balance = false, ahead = false;
  bool fused_tail = true;      // GRX_FETCH_FUSED_TAIL=0: order, commit and gather as launches of their own (FetchVecEnv._fused)
  int slots_per_xcd = 0, split = 1;
  hipStream_t side = nullptr;
  hipEvent_t ev_before = nullptr, ev_ahead = nullptr;
  void* pin[kPinSlots] = {};
  hipEvent_t pin_ev[kPinSlots] = {};
  bool pin_live[kPinSlots] = {};
  size_t pin_bytes = 0;
  int pin_next = 0;
  // host
  std::vector<int64_t> elapsed;
  std::vector<uint8_t> needs_reset, terminated, truncated;
  std::vector<int32_t> final_idx, list, will;
  int n_final = 0;
  uint8_t has_reset = 0;
  // for an attached replay (grx_env_replay.inc): the worlds whose packed row of the last step is the first row of a new episode, as a device index list -- its length on
  // the host, or in device memory where step_count_dev is set -- and the counts of step / reset + set_state calls that order the replay's calls against the handle's
  grx_replay* replay = nullptr;
  grx_norm* norm = nullptr;      // the attached normalizer (grx_env_norm.inc), or none
  const int* step_list = nullptr;
  const int* step_count_dev = nullptr;
  int step_count = 0;
  uint64_t steps = 0, epoch = 0;

  ~grx_env() {
    (void)hipSetDevice(device);
    if (side) (void)hipStreamSynchronize(side);
    (void)hipDeviceSynchronize();
    for (int s = 0; s < kPinSlots; ++s) {
      if (pin_ev[s]) (void)hipEventDestroy(pin_ev[s]);
      if (pin[s]) (void)hipHostFree(pin[s]);
    }
    if (ev_before) (void)hipEventDestroy(ev_before);
    if (ev_ahead) (void)hipEventDestroy(ev_ahead);
    if (side) (void)hipStreamDestroy(side);
    for (void* p : allocs) (void)hipFree(p);
    if (h) grx_model_destroy(h);
    if (hbig) grx_model_destroy(hbig);
    maze_free(mz);
  }

  template <class T>
  int zalloc(T** p, size_t count) {
    void* q = nullptr;
    ENV_HIP(hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 1));
    allocs.push_back(q);
    ENV_HIP(hipMemset(q, 0, count * sizeof(T)));
    *p = (T*)q;
    return 0;
  }

  // host -> device through the pinned ring: enqueued, never waited for (a slot is reused sixteen uploads later, its copy event checked first)
  int upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return 0;
    const int k = pin_next;
    pin_next = (pin_next + 1) % kPinSlots;
    if (pin_live[k] && hipEventQuery(pin_ev[k]) == hipErrorNotReady) ENV_HIP(hipEventSynchronize(pin_ev[k]));
    std::memcpy(pin[k], src, bytes);
    ENV_HIP(hipMemcpyAsync(dst, pin[k], bytes, hipMemcpyHostToDevice, s));
    ENV_HIP(hipEventRecord(pin_ev[k], s));
    pin_live[k] = true;
    return 0;
  }
};

namespace {

struct DeviceGuard {      // the handle's device for the duration of a call, the caller's afterwards
  int prev = -1;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
  ~DeviceGuard() { int cur; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); }
};

grx_fetch_buffers make_bufs(grx_env* e, float* qpos, float* qvel, float* qacc, float* mocap, float* aux, float* goal, float* obs, float* ach, float* rew, unsigned char* succ,
                            int* status, const unsigned char* mask, const int* order, int* cost, float* packed, float* hullcache) {
  grx_fetch_buffers b;
  std::memset(&b, 0, sizeof b);
  b.qpos = qpos; b.qvel = qvel; b.qacc_ws = qacc; b.mocap = mocap; b.aux = aux; b.goal = goal; b.action = e->action; b.obs = obs; b.achieved = ach;
  b.reward = rew; b.success = succ; b.status = status; b.mask = mask; b.order = order; b.cost = cost; b.packed = packed; b.hullcache = hullcache;
  return b;
}

// core.OverflowLane.rerun_only: the step launch with the entry list armed, then the large tables over the worlds that overflowed; then the next order (FetchVecEnv._launch_step)
int launch_step(grx_env* e, bool masked, bool order_now, hipStream_t s) {
  grx_fetch_buffers& fb = masked ? e->bufs_masked : e->bufs;
  ENV_HIP(hipMemsetAsync(e->lane_head, 0, e->lane_head_bytes, s));
  int* counts = e->lane_head + (e->lane_head_bytes / 4 - 2);      // next_count, entry_count
  std::memset(&fb.lane, 0, sizeof fb.lane);
  fb.lane.entry_count = counts + 1; fb.lane.entry_list = e->lane_entry_list; fb.lane.entry_cap = kEntryCap;
  const int rc = grx_fetch_step(e->h, &e->d.task, &fb, e->n, s);
  std::memset(&fb.lane, 0, sizeof fb.lane);
  if (rc != 0) return fail(GRX_ENV_EHIP, std::string("grx_fetch_step: ") + grx_last_error());
  grx_fetch_buffers& b = masked ? e->lane_masked : e->lane_plain;
  std::memset(&b.lane, 0, sizeof b.lane);
  b.lane.grid = kEntryCap; b.lane.list = e->lane_entry_list; b.lane.count = counts + 1;
  b.lane.next_flags = (unsigned char*)e->lane_head; b.lane.next_count = counts; b.lane.next_list = e->lane_next_list; b.lane.ttl = e->lane_ttl; b.lane.next_cap = 0;
  b.lane.soft_maxefc = e->soft[0]; b.lane.soft_jpool = e->soft[1]; b.lane.soft_maxcon = e->soft[2]; b.lane.ttl_init = e->soft[3];
  ENV_GRX(grx_fetch_step(e->hbig, &e->d.task, &b, e->n, s));
  if (e->balance && order_now) ENV_GRX(grx_order_by_cost_slots(e->cost, e->cost_ema, kBalanceAlpha, e->n, e->slots_per_xcd, e->order, s));
  return 0;
}

// FetchVecEnv._stage_reset: the device-side PCG64 draws of _reset_sim / _sample_goal for the listed worlds (indices already on the device)
int sample_resets(grx_env* e, const int* idx_dev, int k, float* samples, hipStream_t s) {
  const double* c = e->d.consts;
  ENV_GRX(grx_fetch_sample_resets_device(e->rng, idx_dev, k, (int)c[0], (int)c[2], c[7], c[8], e->toff, e->g0, e->height_offset, samples, s));
  return 0;
}

// FetchVecEnv._launch_reset (in line, on the caller's stream)
int reset_inline(grx_env* e, const int* idx_dev, int k, const float* samples, bool keep_outcome, hipStream_t s) {
  grx_fetch_reset_args a;
  std::memset(&a, 0, sizeof a);
  a.idx = idx_dev; a.samples = samples; a.init_qpos = e->init_qpos; a.init_qvel = e->init_qvel; a.init_mocap = e->init_mocap; a.obj_qadr = e->obj_qadr;
  a.keep_outcome = keep_outcome ? 1 : 0; a.final_packed = keep_outcome ? e->final_packed : nullptr;
  ENV_GRX(grx_fetch_reset(e->h, &e->d.task, &e->bufs, &a, k, s));
  return 0;
}

void mark_reset(grx_env* e, const std::vector<int32_t>& idx) {
  for (int w : idx) { e->elapsed[w] = 0; e->needs_reset[w] = 0; }
}

// FetchVecEnv._env_setup: the two forward passes of fetch_env.py _env_setup on one world -> initial gripper position, height offset, initial state rows
int env_setup(grx_env* e) {
  grx_env one;      // scratch rows of one world (freed with it; no model handles)
  one.device = e->device;
  float *qpos, *qvel, *qacc, *mocap, *aux, *goal, *action, *obs, *ach, *rew, *packed, *hull;
  unsigned char* succ;
  int* status;
  ENV_TRY(one.zalloc(&qpos, e->nq)); ENV_TRY(one.zalloc(&qvel, e->nv)); ENV_TRY(one.zalloc(&qacc, e->nv)); ENV_TRY(one.zalloc(&mocap, 7 * e->nmocap));
  ENV_TRY(one.zalloc(&aux, 8)); ENV_TRY(one.zalloc(&goal, 3)); ENV_TRY(one.zalloc(&action, 4)); ENV_TRY(one.zalloc(&obs, e->obs_dim)); ENV_TRY(one.zalloc(&ach, 3));
  ENV_TRY(one.zalloc(&rew, 1)); ENV_TRY(one.zalloc(&succ, 1)); ENV_TRY(one.zalloc(&status, 1)); ENV_TRY(one.zalloc(&packed, e->pdim)); ENV_TRY(one.zalloc(&hull, kHullWords));
  one.action = action;
  grx_fetch_buffers b = make_bufs(&one, qpos, qvel, qacc, mocap, aux, goal, obs, ach, rew, succ, status, nullptr, nullptr, nullptr, packed, hull);
  std::vector<float> q0(e->d.q0.begin(), e->d.q0.end()), m0(e->d.mocap0.begin(), e->d.mocap0.end());
  ENV_HIP(hipMemcpy(qpos, q0.data(), q0.size() * 4, hipMemcpyHostToDevice));
  ENV_HIP(hipMemcpy(mocap, m0.data(), m0.size() * 4, hipMemcpyHostToDevice));
  hipStream_t s = e->side;
  ENV_GRX(grx_fetch_forward(e->h, &e->d.task, &b, 1, 0, s));
  ENV_HIP(hipStreamSynchronize(s));
  float o[3];
  ENV_HIP(hipMemcpy(o, obs, 12, hipMemcpyDeviceToHost));
  const double geh = e->d.consts[3];
  const double target[3] = {-0.498 + (double)o[0], 0.005 + (double)o[1], (-0.431 + geh) + (double)o[2]};
  const float mrow[7] = {(float)target[0], (float)target[1], (float)target[2], 1.0f, 0.0f, 1.0f, 0.0f};
  ENV_HIP(hipMemcpy(mocap, mrow, sizeof mrow, hipMemcpyHostToDevice));
  ENV_GRX(grx_fetch_forward(e->h, &e->d.task, &b, 1, 10 * e->d.task.n_substeps, s));
  ENV_HIP(hipStreamSynchronize(s));
  int st = 0;
  float a[3];
  ENV_HIP(hipMemcpy(&st, status, 4, hipMemcpyDeviceToHost));
  if (st != 0) return fail(GRX_ENV_EHIP, "engine reported status " + std::to_string(st) + " during env setup");
  ENV_HIP(hipMemcpy(o, obs, 12, hipMemcpyDeviceToHost));
  ENV_HIP(hipMemcpy(a, ach, 12, hipMemcpyDeviceToHost));
  for (int i = 0; i < 3; ++i) e->g0[i] = (double)o[i];
  e->height_offset = e->d.consts[0] != 0.0 ? (double)a[2] : 0.0;
  ENV_HIP(hipMemcpy(e->init_qpos, qpos, e->nq * 4, hipMemcpyDeviceToDevice));
  ENV_HIP(hipMemcpy(e->init_qvel, qvel, e->nv * 4, hipMemcpyDeviceToDevice));
  ENV_HIP(hipMemcpy(e->init_mocap, m0.data(), m0.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

int alloc_all(grx_env* e) {
  const int n = e->n;
  ENV_TRY(e->zalloc(&e->qpos, (size_t)n * e->nq)); ENV_TRY(e->zalloc(&e->qvel, (size_t)n * e->nv)); ENV_TRY(e->zalloc(&e->qacc_ws, (size_t)n * e->nv));
  ENV_TRY(e->zalloc(&e->mocap, (size_t)n * 7 * e->nmocap)); ENV_TRY(e->zalloc(&e->aux, (size_t)n * 8)); ENV_TRY(e->zalloc(&e->goal, (size_t)n * 3));
  ENV_TRY(e->zalloc(&e->action, (size_t)n * 4)); ENV_TRY(e->zalloc(&e->obs, (size_t)n * e->obs_dim)); ENV_TRY(e->zalloc(&e->achieved, (size_t)n * 3));
  ENV_TRY(e->zalloc(&e->reward, n)); ENV_TRY(e->zalloc(&e->success, n)); ENV_TRY(e->zalloc(&e->status, n)); ENV_TRY(e->zalloc(&e->mask, n));
  ENV_HIP(hipMemset(e->mask, 1, n));
  ENV_TRY(e->zalloc(&e->packed, (size_t)n * e->pdim)); ENV_TRY(e->zalloc(&e->final_packed, (size_t)n * e->pdim)); ENV_TRY(e->zalloc(&e->final_rows, (size_t)n * e->pdim));
  ENV_TRY(e->zalloc(&e->hullcache, (size_t)n * kHullWords));
  ENV_TRY(e->zalloc(&e->rng, (size_t)n * 4)); ENV_TRY(e->zalloc(&e->rng_rows, (size_t)n * 4));
  ENV_TRY(e->zalloc(&e->init_qpos, e->nq)); ENV_TRY(e->zalloc(&e->init_qvel, e->nv)); ENV_TRY(e->zalloc(&e->init_mocap, 7 * e->nmocap));
  ENV_TRY(e->zalloc(&e->idx_main, n)); ENV_TRY(e->zalloc(&e->idx_ahead, n)); ENV_TRY(e->zalloc(&e->samp_main, (size_t)n * 5)); ENV_TRY(e->zalloc(&e->samp_ahead, (size_t)n * 5));
  e->lane_head_bytes = (size_t)((n + 3) / 4 + 2) * 4;
  ENV_TRY(e->zalloc(&e->lane_head, e->lane_head_bytes / 4)); ENV_TRY(e->zalloc(&e->lane_next_list, n)); ENV_TRY(e->zalloc(&e->lane_entry_list, n)); ENV_TRY(e->zalloc(&e->lane_ttl, n));
  // cost-ordered dispatch (FetchVecEnv._alloc): a multiple of 8 worlds, one XCD slice per sorting workgroup
  e->balance = n % 8 == 0 && n >= 1024 && n <= 65536 * 8;
  { const char* v = std::getenv("GRX_FETCH_FUSED_TAIL"); e->fused_tail = !(v && v[0] == '0' && v[1] == 0); }
  if (e->balance) {
    ENV_TRY(e->zalloc(&e->cost, n)); ENV_TRY(e->zalloc(&e->cost_ema, n)); ENV_TRY(e->zalloc(&e->order, n));
    const int lds = grx_model_lds_bytes(e->h);
    const int granules = (lds + 1279) / 1280;
    const int per_cu = granules > 0 ? (160 * 1024) / (granules * 1280) : 8;
    e->slots_per_xcd = 32 * (per_cu < 8 ? per_cu : 8);
    std::vector<int> ord(n);
    const int per = n / 8;
    for (int j = 0; j < n; ++j) ord[j] = (j % 8) * per + j / 8;      // workgroup j -> XCD slice j & 7, position j >> 3
    ENV_HIP(hipMemcpy(e->order, ord.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  e->bufs = make_bufs(e, e->qpos, e->qvel, e->qacc_ws, e->mocap, e->aux, e->goal, e->obs, e->achieved, e->reward, e->success, e->status, nullptr, e->order, e->cost, e->packed, e->hullcache);
  e->bufs_masked = e->bufs;
  e->bufs_masked.mask = e->mask;
  e->lane_plain = make_bufs(e, e->qpos, e->qvel, e->qacc_ws, e->mocap, e->aux, e->goal, e->obs, e->achieved, e->reward, e->success, e->status, nullptr, nullptr, nullptr, e->packed,
                            e->hullcache);
  e->lane_masked = e->lane_plain;
  e->lane_masked.mask = e->mask;
  // split step: 4 parts above one round of wave slots, 2 above FETCH_SPLIT_WIDE
  e->split = n >= 64 && n > 2048 ? (n <= kSplitWide ? kSplitParts : 2) : 1;
  if (e->split > 1) {
    const int stride = (2 + e->nu + 7 * e->nmocap + e->nq + 2 * e->nv + 15) / 16 * 16;
    ENV_TRY(e->zalloc(&e->split_rows, (size_t)n * stride)); ENV_TRY(e->zalloc(&e->split_state, (size_t)n * 2));
    for (grx_fetch_buffers* b : {&e->bufs, &e->bufs_masked}) { b->handoff = e->split_rows; b->handoff_stride = stride; b->split_state = e->split_state; b->split_parts = e->split; }
  }
  // the staged rows of the same-step reset that runs beside the step launch
  e->ahead = n > 1;
  if (e->ahead) {
    ENV_TRY(e->zalloc(&e->a_qpos, (size_t)n * e->nq)); ENV_TRY(e->zalloc(&e->a_qvel, (size_t)n * e->nv)); ENV_TRY(e->zalloc(&e->a_qacc_ws, (size_t)n * e->nv));
    ENV_TRY(e->zalloc(&e->a_mocap, (size_t)n * 7 * e->nmocap)); ENV_TRY(e->zalloc(&e->a_aux, (size_t)n * 8)); ENV_TRY(e->zalloc(&e->a_goal, (size_t)n * 3));
    ENV_TRY(e->zalloc(&e->a_obs, (size_t)n * e->obs_dim)); ENV_TRY(e->zalloc(&e->a_achieved, (size_t)n * 3)); ENV_TRY(e->zalloc(&e->a_reward, n));
    ENV_TRY(e->zalloc(&e->a_success, n)); ENV_TRY(e->zalloc(&e->a_status, n));
    e->ahead_bufs = make_bufs(e, e->a_qpos, e->a_qvel, e->a_qacc_ws, e->a_mocap, e->a_aux, e->a_goal, e->a_obs, e->a_achieved, e->a_reward, e->a_success, e->a_status, nullptr,
                              nullptr, nullptr, nullptr, nullptr);
  }
  e->pin_bytes = (size_t)n * 32;      // an index list (int32 [N]) or a block of stream rows (uint64 [N, 4])
  for (int s = 0; s < kPinSlots; ++s) {
    ENV_HIP(hipHostMalloc(&e->pin[s], e->pin_bytes, hipHostMallocDefault));
    ENV_HIP(hipEventCreateWithFlags(&e->pin_ev[s], hipEventDisableTiming));
  }
  ENV_HIP(hipEventCreateWithFlags(&e->ev_before, hipEventDisableTiming));
  ENV_HIP(hipEventCreateWithFlags(&e->ev_ahead, hipEventDisableTiming));
  e->elapsed.assign(n, 0);
  e->needs_reset.assign(n, 0);
  e->terminated.assign(n, 0);
  e->truncated.assign(n, 0);
  e->final_idx.reserve(n);
  e->list.reserve(n);
  e->will.reserve(n);
  return 0;
}

// the device rows and host arrays of a state blob, in blob order
struct Section { const char* name; void* ptr; size_t bytes; bool host; };

#include "grx_env_maze.inc"

std::vector<Section> maze_sections(grx_env* e) {
  MazeEnv& m = *e->mz;
  const size_t n = e->n;
  std::vector<Section> s = {
      {"qpos", m.qpos, n * m.nq * 4, false}, {"qvel", m.qvel, n * m.nv * 4, false}, {"qacc_ws", m.qacc_ws, n * m.nv * 4, false}, {"goal", m.goal, n * 8, false},
      {"obs", m.obs, n * e->obs_dim * 4, false}, {"achieved", m.achieved, n * 8, false}, {"reward", m.reward, n * 4, false}, {"success", m.success, n, false},
      {"status", m.status, n * 4, false}, {"packed", m.packed, n * e->pdim * 4, false}, {"desired", m.desired, n * 8, false}, {"rng", m.rng, n * 40, false},
      {"mask", m.mask, n, false}};
  // the time-limit counters: on the host where the host keeps them (MazeEnv::host_book), else the device's
  if (m.host_book) { s.push_back({"elapsed", m.h_elapsed.data(), n * 8, true}); s.push_back({"needs_reset", m.h_needs_reset.data(), n, true}); }
  else { s.push_back({"elapsed", m.elapsed, n * 8, false}); s.push_back({"needs_reset", m.needs_reset, n, false}); }
  if (m.split > 1) s.push_back({"split_state", m.split_state, n * 8, false});
  s.push_back({"has_reset", &e->has_reset, 1, true});
  return s;
}

std::vector<Section> state_sections(grx_env* e) {
  if (e->mz) return maze_sections(e);
  const size_t n = e->n;
  std::vector<Section> s = {
      {"qpos", e->qpos, n * e->nq * 4, false}, {"qvel", e->qvel, n * e->nv * 4, false}, {"qacc_ws", e->qacc_ws, n * e->nv * 4, false},
      {"mocap", e->mocap, n * 7 * e->nmocap * 4, false}, {"aux", e->aux, n * 8 * 4, false}, {"goal", e->goal, n * 3 * 4, false},
      {"obs", e->obs, n * e->obs_dim * 4, false}, {"achieved", e->achieved, n * 3 * 4, false}, {"reward", e->reward, n * 4, false},
      {"success", e->success, n, false}, {"status", e->status, n * 4, false}, {"packed", e->packed, n * e->pdim * 4, false},
      {"final_packed", e->final_packed, n * e->pdim * 4, false}, {"rng", e->rng, n * 32, false}, {"hullcache", e->hullcache, n * kHullWords * 4, false}};
  if (e->balance) {
    s.push_back({"cost", e->cost, n * 4, false});
    s.push_back({"cost_ema", e->cost_ema, n * 4, false});
    s.push_back({"order", e->order, n * 4, false});
  }
  s.push_back({"elapsed", e->elapsed.data(), n * 8, true});
  s.push_back({"needs_reset", e->needs_reset.data(), n, true});
  s.push_back({"has_reset", &e->has_reset, 1, true});
  return s;
}

size_t state_layout(grx_env* e, std::vector<uint64_t>* offsets) {
  auto secs = state_sections(e);
  uint64_t off = sizeof(Header) + secs.size() * sizeof(Entry);
  for (auto& s : secs) {
    off = (off + 7) / 8 * 8;
    if (offsets) offsets->push_back(off);
    off += s.bytes;
  }
  return off;
}

}  // namespace

// ------------------------------------------------------------------ entry points
extern "C" const char* grx_env_last_error(void) { return g_err.c_str(); }

extern "C" int grx_env_seed_pcg64(const uint64_t* seeds, int n, uint64_t* states) {
  if ((!seeds || !states) && n > 0) return fail(GRX_ENV_EINVAL, "grx_env_seed_pcg64: null argument");
  if (n < 0) return fail(GRX_ENV_EINVAL, "grx_env_seed_pcg64: negative count");
  for (int i = 0; i < n; ++i) pcg64_from_seed(seeds[i], states + 4 * (size_t)i);
  return 0;
}

extern "C" int grx_env_create(const char* desc_path, int num_envs, int device, const grx_env_config* cfg, grx_env** out) {
  if (!out) return fail(GRX_ENV_EINVAL, "grx_env_create: out is NULL");
  *out = nullptr;
  if (!desc_path) return fail(GRX_ENV_EINVAL, "grx_env_create: desc_path is NULL");
  if (num_envs <= 0 || num_envs > (1 << 24)) return fail(GRX_ENV_EINVAL, "grx_env_create: num_envs " + std::to_string(num_envs) + " out of range");
  if (cfg && (cfg->autoreset_mode < 0 || cfg->autoreset_mode > 2)) return fail(GRX_ENV_EINVAL, "grx_env_create: unknown autoreset_mode " + std::to_string(cfg->autoreset_mode));
  grx_env* e = new grx_env();
  e->n = num_envs;
  e->device = device;
  int rc = [&]() -> int {      // the whole file, before the device is touched
    std::vector<uint8_t> buf;
    Container c;
    std::string family;
    ENV_TRY(read_desc(desc_path, &buf, &c));
    e->d.env_id = c.h.env_id;
    if (desc_is_maze(c, &family)) {
      e->mz = new MazeEnv();
      return parse_maze_desc(c, &e->mz->d);
    }
    if (family != "fetch") return fail(GRX_ENV_EDESC, "environment description: unknown family '" + family + "' (this library reads fetch and maze descriptions)");
    return parse_desc(c, &e->d);
  }();
  if (rc != 0) { std::string msg = g_err; delete e; g_err = msg; return rc; }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { delete e; return fail(GRX_ENV_ENODEV, "grx_env_create: no HIP device"); }
  if (device < 0 || device >= count) { delete e; return fail(GRX_ENV_ENODEV, "grx_env_create: no HIP device " + std::to_string(device) + " (" + std::to_string(count) + " visible)"); }
  DeviceGuard g(device);
  if (e->mz) {
    rc = maze_create(e, cfg);
    if (rc != 0) {
      std::string msg = g_err;
      delete e;
      g_err = msg;
      return rc;
    }
    *out = e;
    return 0;
  }
  const Desc& d = e->d;
  e->nq = d.dims[0]; e->nv = d.dims[1]; e->nmocap = d.dims[2]; e->nu = d.dims[3]; e->obs_dim = d.dims[4]; e->obj_qadr = d.dims[5];
  e->pdim = e->obs_dim + 8;
  e->mode = cfg ? cfg->autoreset_mode : GRX_ENV_NEXT_STEP;
  e->max_steps = cfg ? (cfg->max_episode_steps > 0 ? cfg->max_episode_steps : 0) : d.dims[6];
  e->seed_offset = cfg ? cfg->seed_offset : 0;
  for (int i = 0; i < 3; ++i) e->toff[i] = d.consts[4 + i];
  e->dt = d.consts[10];
  const int caps[3] = {d.caps[0], d.caps[1], d.caps[2] < 32 ? d.caps[2] : 32};      // core.OverflowLane: int(margin * capacity), at most 32 contacts
  for (int i = 0; i < 3; ++i) e->soft[i] = (int)(kLaneMargin * caps[i]);
  e->soft[3] = kLaneTtl;
  rc = [&]() -> int {
    ENV_GRX(grx_model_create(d.H.data(), (int)d.H.size(), d.I.data(), (int)d.I.size(), d.F.data(), (int)d.F.size(), device, &e->h));
    ENV_GRX(grx_model_create(d.Hr.data(), (int)d.Hr.size(), d.Ir.data(), (int)d.Ir.size(), d.Fr.data(), (int)d.Fr.size(), device, &e->hbig));
    if (grx_model_dim(e->h, "nq") != e->nq || grx_model_dim(e->h, "nv") != e->nv || grx_model_dim(e->h, "nmocap") != e->nmocap || grx_model_dim(e->h, "nu") != e->nu)
      return fail(GRX_ENV_EDESC, "environment description: inconsistent sizes: the model tables disagree with dims");
    ENV_HIP(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
    ENV_TRY(alloc_all(e));
    ENV_TRY(env_setup(e));
    std::vector<uint64_t> st((size_t)e->n * 4);      // every world: SeedSequence(None)
    for (int i = 0; i < e->n; ++i) ENV_TRY(pcg64_from_os(&st[(size_t)i * 4]));
    ENV_HIP(hipMemcpy(e->rng, st.data(), st.size() * 8, hipMemcpyHostToDevice));
    ENV_HIP(hipDeviceSynchronize());
    return 0;
  }();
  if (rc != 0) {
    std::string msg = g_err;
    delete e;
    g_err = msg;
    return rc;
  }
  *out = e;
  return 0;
}

extern "C" int grx_env_destroy(grx_env* e) {
  if (!e) return fail(GRX_ENV_EINVAL, "grx_env_destroy: NULL handle");
  if (e->replay) return fail(GRX_ENV_EINVAL, "grx_env_destroy: a replay is attached to the handle: grx_replay_destroy first");
  if (e->norm) return fail(GRX_ENV_EINVAL, "grx_env_destroy: a normalizer is attached to the handle: grx_norm_destroy first");
  delete e;
  return 0;
}

extern "C" int grx_env_dims(const grx_env* e, int* obs_dim, int* goal_dim, int* act_dim, double* dt) {
  if (!e) return fail(GRX_ENV_EINVAL, "grx_env_dims: NULL handle");
  if (obs_dim) *obs_dim = e->obs_dim;
  if (goal_dim) *goal_dim = e->mz ? 2 : 3;
  if (act_dim) *act_dim = e->mz ? e->mz->nu : 4;
  if (dt) *dt = e->dt;
  return 0;
}

extern "C" int grx_env_reset(grx_env* e, const uint8_t* mask, const uint64_t* seeds, void* stream) {
  if (!e) return fail(GRX_ENV_EINVAL, "grx_env_reset: NULL handle");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  e->epoch += 1;
  e->step_list = nullptr; e->step_count_dev = nullptr; e->step_count = 0;
  if (e->mz) return maze_reset(e, mask, seeds, s);
  auto& L = e->list;
  L.clear();
  for (int i = 0; i < e->n; ++i)
    if (!mask || mask[i]) L.push_back(i);
  e->n_final = 0;
  std::fill(e->terminated.begin(), e->terminated.end(), 0);
  std::fill(e->truncated.begin(), e->truncated.end(), 0);
  e->has_reset = 1;
  const int k = (int)L.size();
  if (k == 0) return 0;
  ENV_TRY(e->upload(e->idx_main, L.data(), (size_t)k * 4, s));
  if (seeds) {      // the listed worlds' streams: PCG64(SeedSequence(seeds[i]))
    std::vector<uint64_t> rows((size_t)k * 4);
    for (int j = 0; j < k; ++j) pcg64_from_seed(seeds[L[j]], &rows[(size_t)j * 4]);
    ENV_TRY(e->upload(e->rng_rows, rows.data(), rows.size() * 8, s));
    hipLaunchKernelGGL(grx_env_scatter_rng_kernel, dim3(blocks(k)), dim3(64), 0, s, (unsigned long long*)e->rng, (const unsigned long long*)e->rng_rows, e->idx_main, k);
    ENV_HIP(hipGetLastError());
  }
  ENV_TRY(sample_resets(e, e->idx_main, k, e->samp_main, s));
  ENV_TRY(reset_inline(e, e->idx_main, k, e->samp_main, false, s));
  mark_reset(e, L);
  return 0;
}

extern "C" int grx_env_step(grx_env* e, const float* actions, void* stream) {
  if (!e) return fail(GRX_ENV_EINVAL, "grx_env_step: NULL handle");
  if (!actions) return fail(GRX_ENV_EINVAL, "grx_env_step: actions is NULL");
  if (!e->has_reset) return fail(GRX_ENV_EINVAL, "grx_env_step: cannot step before grx_env_reset");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  e->steps += 1;
  e->step_list = nullptr; e->step_count_dev = nullptr; e->step_count = 0;
  if (e->mz) return maze_step(e, actions, s);
  const int n = e->n;
  ENV_HIP(hipMemcpyAsync(e->action, actions, (size_t)n * 16, hipMemcpyDefault, s));
  auto& pending = e->list;
  pending.clear();
  if (e->mode == GRX_ENV_NEXT_STEP)
    for (int i = 0; i < n; ++i)
      if (e->needs_reset[i]) pending.push_back(i);
  auto& will = e->will;      // the worlds this step truncates (Fetch has no other episode end): reset ahead, beside the step launch
  will.clear();
  if (e->ahead && e->mode == GRX_ENV_SAME_STEP && e->max_steps > 0)
    for (int i = 0; i < n; ++i)
      if (e->elapsed[i] + 1 >= e->max_steps) will.push_back(i);
  const int kp = (int)pending.size(), kw = (int)will.size();
  if (kw) ENV_HIP(hipEventRecord(e->ev_before, s));      // the side stream waits for what is queued now, not for the step launch that follows
  if (kp) {
    ENV_TRY(e->upload(e->idx_main, pending.data(), (size_t)kp * 4, s));
    ENV_HIP(hipMemsetAsync(e->mask, 1, n, s));
    hipLaunchKernelGGL(grx_env_mask_kernel, dim3(blocks(kp)), dim3(64), 0, s, e->mask, (const int*)e->idx_main, kp);
    ENV_HIP(hipGetLastError());
  }
  // fused tail (grx_fetch_post_step): in same-step mode the next order is sorted by the launch that commits the reset rows (the step's costs are final once it has ended)
  const bool post = e->fused_tail && e->mode == GRX_ENV_SAME_STEP && kp == 0;
  bool ordered = !(post && e->balance);
  ENV_TRY(launch_step(e, kp > 0, !post, s));
  if (kw) {      // queued behind the step launch: its workgroups take the wave slots the first finished worlds free
    ENV_HIP(hipStreamWaitEvent(e->side, e->ev_before, 0));
    ENV_TRY(e->upload(e->idx_ahead, will.data(), (size_t)kw * 4, e->side));
    ENV_TRY(sample_resets(e, e->idx_ahead, kw, e->samp_ahead, e->side));
    grx_fetch_reset_args a;
    std::memset(&a, 0, sizeof a);
    a.idx = e->idx_ahead; a.samples = e->samp_ahead; a.init_qpos = e->init_qpos; a.init_qvel = e->init_qvel; a.init_mocap = e->init_mocap; a.obj_qadr = e->obj_qadr;
    a.keep_outcome = 1; a.final_packed = nullptr;
    ENV_GRX(grx_fetch_reset(e->h, &e->d.task, &e->ahead_bufs, &a, kw, e->side));
    ENV_HIP(hipEventRecord(e->ev_ahead, e->side));
  }
  // time limit (FetchVecEnv.step): the worlds reset in place of this step do not count it
  e->n_final = 0;
  e->final_idx.clear();
  for (int i = 0; i < n; ++i) {
    const bool stepped = !(kp && e->needs_reset[i]);
    if (stepped) e->elapsed[i] += 1;
    e->truncated[i] = stepped && e->max_steps > 0 && e->elapsed[i] >= e->max_steps;
    e->terminated[i] = 0;
    if (e->truncated[i]) e->final_idx.push_back(i);
  }
  if (kp) {      // next-step autoreset: the reset replaces the step, reward 0 and flags False
    ENV_TRY(sample_resets(e, e->idx_main, kp, e->samp_main, s));
    ENV_TRY(reset_inline(e, e->idx_main, kp, e->samp_main, false, s));
    mark_reset(e, pending);
    e->step_list = e->idx_main; e->step_count = kp;
    hipLaunchKernelGGL(grx_env_zero_outcome_kernel, dim3(blocks(kp)), dim3(64), 0, s, e->reward, e->packed, e->pdim, (const int*)e->idx_main, kp);
    ENV_HIP(hipGetLastError());
  }
  const int kd = (int)e->final_idx.size();
  bool gathered = false;
  if (e->mode == GRX_ENV_SAME_STEP && kd) {
    const int* idx_dev;
    if (kw) {
      if (kw != kd || !std::equal(will.begin(), will.end(), e->final_idx.begin())) {
        if (!ordered) (void)grx_fetch_post_step(e->cost, e->cost_ema, kBalanceAlpha, e->n, e->slots_per_xcd, e->order, nullptr, nullptr, s);      // nothing is committed: the order alone
        return fail(GRX_ENV_EINVAL, "grx_env_step: the worlds reset ahead of the step are not the ones it truncated");
      }
      ENV_HIP(hipStreamWaitEvent(s, e->ev_ahead, 0));
      grx_fetch_commit_args c;
      std::memset(&c, 0, sizeof c);
      c.idx = e->idx_ahead; c.k = kd; c.nq = e->nq; c.nv = e->nv; c.mocap_words = 7 * e->nmocap; c.obs_dim = e->obs_dim;
      c.s_qpos = e->a_qpos; c.s_qvel = e->a_qvel; c.s_qacc_ws = e->a_qacc_ws; c.s_mocap = e->a_mocap; c.s_aux = e->a_aux; c.s_goal = e->a_goal; c.s_obs = e->a_obs;
      c.s_achieved = e->a_achieved; c.s_status = e->a_status;
      c.qpos = e->qpos; c.qvel = e->qvel; c.qacc_ws = e->qacc_ws; c.mocap = e->mocap; c.aux = e->aux; c.goal = e->goal; c.obs = e->obs; c.achieved = e->achieved;
      c.packed = e->packed; c.final_packed = e->final_packed; c.status = e->status;
      if (post) {
        ENV_GRX(grx_fetch_post_step(e->cost, e->cost_ema, kBalanceAlpha, e->n, e->slots_per_xcd, e->balance ? e->order : nullptr, &c, e->final_rows, s));
        ordered = gathered = true;
      } else ENV_GRX(grx_fetch_commit_rows(&c, s));
      idx_dev = e->idx_ahead;
    } else {      // one world (no side stream): the in-line reset parks the terminal rows itself
      ENV_TRY(e->upload(e->idx_main, e->final_idx.data(), (size_t)kd * 4, s));
      ENV_TRY(sample_resets(e, e->idx_main, kd, e->samp_main, s));
      ENV_TRY(reset_inline(e, e->idx_main, kd, e->samp_main, true, s));
      idx_dev = e->idx_main;
    }
    mark_reset(e, e->final_idx);
    if (!gathered) {
      hipLaunchKernelGGL(grx_env_gather_kernel, dim3(blocks(kd)), dim3(64), 0, s, e->final_rows, (const float*)e->final_packed, e->pdim, idx_dev, kd);
      ENV_HIP(hipGetLastError());
    }
    e->n_final = kd;
    e->step_list = idx_dev; e->step_count = kd;
  } else {
    if (e->mode == GRX_ENV_NEXT_STEP)
      for (int w : e->final_idx) e->needs_reset[w] = 1;
    e->final_idx.clear();
  }
  if (!ordered) ENV_GRX(grx_fetch_post_step(e->cost, e->cost_ema, kBalanceAlpha, e->n, e->slots_per_xcd, e->order, nullptr, nullptr, s));      // no world ended (or one world, reset in line)
  return 0;
}

extern "C" int grx_env_outputs(const grx_env* e, grx_env_device_outputs* out) {
  if (!e || !out) return fail(GRX_ENV_EINVAL, "grx_env_outputs: NULL argument");
  if (e->mz) return maze_outputs(e, out);
  out->num_envs = e->n; out->obs_dim = e->obs_dim; out->goal_dim = 3; out->packed_dim = e->pdim;
  out->obs = e->obs; out->achieved = e->achieved; out->desired = e->goal; out->reward = e->reward; out->success = e->success; out->status = e->status; out->packed = e->packed;
  out->terminated = e->terminated.data(); out->truncated = e->truncated.data();
  out->n_final = e->n_final; out->final_idx = e->final_idx.data(); out->final_rows = e->final_rows;
  return 0;
}

extern "C" int grx_env_copy_outputs(grx_env* e, grx_env_host_outputs* out) {
  if (!e || !out) return fail(GRX_ENV_EINVAL, "grx_env_copy_outputs: NULL argument");
  DeviceGuard g(e->device);
  if (e->mz) return maze_copy_outputs(e, out);
  ENV_HIP(hipDeviceSynchronize());
  const size_t n = e->n;
  auto d2h = [](void* dst, const void* src, size_t bytes) { return (dst && bytes) ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
  ENV_HIP(d2h(out->obs, e->obs, n * e->obs_dim * 4));
  ENV_HIP(d2h(out->achieved, e->achieved, n * 12));
  ENV_HIP(d2h(out->desired, e->goal, n * 12));
  ENV_HIP(d2h(out->reward, e->reward, n * 4));
  ENV_HIP(d2h(out->success, e->success, n));
  ENV_HIP(d2h(out->status, e->status, n * 4));
  ENV_HIP(d2h(out->packed, e->packed, n * e->pdim * 4));
  ENV_HIP(d2h(out->final_rows, e->final_rows, (size_t)e->n_final * e->pdim * 4));
  if (out->terminated) std::memcpy(out->terminated, e->terminated.data(), n);
  if (out->truncated) std::memcpy(out->truncated, e->truncated.data(), n);
  if (out->n_final) *out->n_final = e->n_final;
  if (out->final_idx && e->n_final) std::memcpy(out->final_idx, e->final_idx.data(), (size_t)e->n_final * 4);
  return 0;
}

extern "C" int grx_env_compute_reward(const grx_env* e, const float* achieved, const float* desired, int64_t batch, float* out, void* stream) {
  if (!e || !achieved || !desired || !out) return fail(GRX_ENV_EINVAL, "grx_env_compute_reward: NULL argument");
  if (batch < 0) return fail(GRX_ENV_EINVAL, "grx_env_compute_reward: negative batch");
  DeviceGuard g(e->device);
  if (e->mz) {
    ENV_GRX(grx_maze_compute_reward(achieved, desired, batch, e->mz->d.task.goal_radius, e->mz->d.task.sparse_reward, out, stream));
    return 0;
  }
  ENV_GRX(grx_fetch_compute_reward(achieved, desired, batch, e->d.task.distance_threshold, e->d.task.sparse_reward, out, stream));
  return 0;
}

extern "C" int grx_env_state_size(const grx_env* e, size_t* bytes) {
  if (!e || !bytes) return fail(GRX_ENV_EINVAL, "grx_env_state_size: NULL argument");
  *bytes = state_layout(const_cast<grx_env*>(e), nullptr);
  return 0;
}

extern "C" int grx_env_get_state(grx_env* e, void* host, size_t bytes) {
  if (!e || !host) return fail(GRX_ENV_EINVAL, "grx_env_get_state: NULL argument");
  std::vector<uint64_t> off;
  const size_t total = state_layout(e, &off);
  if (bytes < total) return fail(GRX_ENV_EINVAL, "grx_env_get_state: buffer of " + std::to_string(bytes) + " bytes, the state needs " + std::to_string(total));
  DeviceGuard g(e->device);
  ENV_HIP(hipDeviceSynchronize());
  uint8_t* p = (uint8_t*)host;
  std::memset(p, 0, total);
  auto secs = state_sections(e);
  Header h;
  std::memset(&h, 0, sizeof h);
  std::memcpy(h.magic, kStateMagic, 8);
  h.version = GRX_ENV_STATE_VERSION; h.n_sections = (uint32_t)secs.size(); h.num_envs = e->n; h.total_bytes = total;
  std::strncpy(h.env_id, e->d.env_id.c_str(), sizeof h.env_id - 1);
  std::memcpy(p, &h, sizeof h);
  for (size_t k = 0; k < secs.size(); ++k) {
    Entry en;
    std::memset(&en, 0, sizeof en);
    std::strncpy(en.name, secs[k].name, sizeof en.name - 1);
    en.offset = off[k]; en.bytes = secs[k].bytes;
    std::memcpy(p + sizeof(Header) + k * sizeof(Entry), &en, sizeof en);
    if (secs[k].host) std::memcpy(p + off[k], secs[k].ptr, secs[k].bytes);
    else ENV_HIP(hipMemcpy(p + off[k], secs[k].ptr, secs[k].bytes, hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int grx_env_set_state(grx_env* e, const void* host, size_t bytes) {
  if (!e || !host) return fail(GRX_ENV_EINVAL, "grx_env_set_state: NULL argument");
  Container c;
  ENV_TRY(parse_container((const uint8_t*)host, bytes, kStateMagic, GRX_ENV_STATE_VERSION, "state blob", GRX_ENV_ESTATE, &c));
  c.h.env_id[47] = 0;
  if (e->d.env_id != c.h.env_id || c.h.num_envs != e->n)
    return fail(GRX_ENV_ESTATE, std::string("state blob of ") + c.h.env_id + " x " + std::to_string(c.h.num_envs) + " does not fit " + e->d.env_id + " x " + std::to_string(e->n));
  auto secs = state_sections(e);
  for (auto& s : secs) {      // every section present and of this handle's size before anything is written
    auto it = c.sec.find(s.name);
    if (it == c.sec.end()) return fail(GRX_ENV_ESTATE, std::string("state blob: section '") + s.name + "' is missing");
    if (it->second.second != s.bytes)
      return fail(GRX_ENV_ESTATE, std::string("state blob: section '") + s.name + "' holds " + std::to_string(it->second.second) + " bytes, this handle " + std::to_string(s.bytes));
  }
  DeviceGuard g(e->device);
  ENV_HIP(hipDeviceSynchronize());
  for (auto& s : secs) {
    const uint8_t* src = c.sec[s.name].first;
    if (s.host) std::memcpy(s.ptr, src, s.bytes);
    else ENV_HIP(hipMemcpy(s.ptr, src, s.bytes, hipMemcpyHostToDevice));
  }
  ENV_HIP(hipDeviceSynchronize());
  e->has_reset = e->has_reset ? 1 : 0;
  e->epoch += 1;
  e->step_list = nullptr; e->step_count_dev = nullptr; e->step_count = 0;
  if (e->mz) { e->mz->flags_live = false; e->mz->success_parked = false; }
  e->n_final = 0;
  e->final_idx.clear();
  std::fill(e->terminated.begin(), e->terminated.end(), 0);
  std::fill(e->truncated.begin(), e->truncated.end(), 0);
  return 0;
}

#include "grx_env_replay.inc"
#include "grx_env_episodes.inc"
#include "grx_env_norm.inc"
