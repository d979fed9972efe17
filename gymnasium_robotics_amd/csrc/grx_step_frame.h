// grx_step_frame.h -- the frame the five step kernels of grx_kernels.hip share (Fetch, PointMaze / AntMaze, Shadow hand, Adroit, Kitchen): workgroup -> world mapping, the
// overflow lane, the split-step protocol, state rows, the cost stamp and the profiling prologue / epilogue.  Device only; every helper is inlined into its caller.
#pragma once
#include "grx_engine.h"

// ---- world <-> workgroup.  The dispatcher deals workgroups round-robin to the 8 XCDs, each with its own L2, so with w = blockIdx.x the rows of neighbouring worlds (88-B qpos
// rows, 100-B obs rows, 4-B reward / flag entries: several worlds per 128-B line) are fetched by up to 8 L2s and written back as 8 partial lines.  The grid is rounded up to a
// multiple of 8 and XCD k takes the k-th contiguous slice of the worlds, so a line is read and merged in one L2 (rocprofv3 FETCH_SIZE / WRITE_SIZE: profiles/).
// A launch of G slots (split step: `parts` workgroups per world, workgroup index = part * G + slot with G = gridDim.x / parts; slot, slot + G, ... share blockIdx.x mod 8: one
// XCD, one L2 for all parts of a world): the world of a slot, through the cost order (grx_order_kernel) where the launch has one.
static __device__ __forceinline__ int grx_slot_world(const int* order, unsigned slot, unsigned G) { return order ? order[slot] : (int)((slot & 7u) * (G >> 3) + (slot >> 3)); }
// the same index re-derived after the substep loop from the (architected) workgroup id: the epilogue's addresses are then computed there instead of being kept -- as 64-bit
// VGPR pairs spilled to scratch -- across the whole simulation
static __device__ __forceinline__ int grx_slot_world_late(const int* order, int parts) {
  unsigned bx = blockIdx.x; asm volatile("" : "+s"(bx));
  const unsigned G = parts > 1 ? gridDim.x / (unsigned)parts : gridDim.x, slot = parts > 1 ? bx % G : bx;
  return grx_slot_world(order, slot, G);
}

// ---- the overflow lane (include/grx_capi.h, grx_overflow_lane)
// both kernels, before the simulation: the fast kernel may hand the world over at the first overflowing substep (grx_lane_claim, csrc/grx_engine.h), both watch the soft thresholds
__device__ __forceinline__ void grx_lane_setup(const GrxLane& L, GrxCtx& c, int w, bool stepping) {
  c.bail = (stepping && L.entry_count != nullptr) ? 1 : 0;
  if (c.bail) { c.lane_entry_count = L.entry_count; c.lane_entry_list = L.entry_list; c.lane_entry_cap = L.entry_cap; c.lane_world = w; c.lane_ready = L.ready; c.lane_ready_cap = L.ready_cap; }
  if (stepping && (L.list != nullptr || L.entry_count != nullptr)) { c.soft_maxefc = L.soft_maxefc; c.soft_jpool = L.soft_jpool; c.soft_maxcon = L.soft_maxcon; }
}
// fast kernel, after the simulation: true = the world claimed a re-run on the large tables: the caller returns WITHOUT writing anything of it
__device__ __forceinline__ bool grx_lane_overflowed(const GrxCtx& c) { return c.bail == 2; }
// append w to the lane of the next step (both kernels); a full list (next_cap: the grid of the next step's launch) leaves the world on the fast kernel
__device__ __forceinline__ void grx_lane_append(const GrxLane& L, int w) {
  const int idx = atomicAdd(L.next_count, 1);
  if (idx < L.next_cap) { L.next_list[idx] = w; L.next_flags[w] = 1; }
}
// fast kernel, after a step that did NOT overflow but came within the soft thresholds of a capacity: the result is committed as usual and the world moves to the
// lane for the next steps -- before it can overflow, so that entering the lane costs no serialised re-run
__device__ __forceinline__ void grx_lane_join(const GrxLane& L, const GrxCtx& c, int w, int lane_) {
  if (L.entry_count == nullptr || L.next_list == nullptr || lane_ != 0 || !(c.cnt[2] & GRX_ST_SOFT)) return;
  L.ttl[w] = (signed char)L.ttl_init;
  grx_lane_append(L, w);
}
// large-table kernel: the world's ticket (it stays in the lane while it is within the soft thresholds, and ttl_init steps longer); st < 0: the world was not part of this
// step (masked out: it waits for its reset) and keeps its place
__device__ __forceinline__ void grx_lane_ticket(const GrxLane& L, int st, int w, int lane_) {   // st: the world's status flags of this step, -1 = it was not stepped (by value: taking the context's address would keep the whole GrxCtx in scratch memory)
  if (L.list == nullptr || lane_ != 0) return;
  int t = L.ttl[w];
  if (st >= 0) { t = (st & GRX_ST_SOFT) ? L.ttl_init : (t > 0 ? t - 1 : 0); L.ttl[w] = (signed char)t; }
  else if (t <= 0) t = 1;
  if (t > 0) grx_lane_append(L, w);
}
// ---- entrants without the serialised re-run (include/grx_capi.h, grx_overflow_lane.ready / progress / poll_*).  The worlds that overflow are the heaviest of the batch and
// their re-run used to start when the fast launch had ENDED (hand + touch: 2 ms in 60 % of the steps, a hand jammed into the door 5 - 9 ms).  The standing lane launch now
// carries poll_grid extra workgroups; workgroup p sleeps until entry p of THIS step's entry list is published (ready[p] == 1), claims it (-> 2) and steps the world on the
// large tables while the fast launch is still running.  It gives up when every workgroup of the fast launch has ended (progress == progress_total) or after a bounded number
// of polls; whatever is unclaimed then is taken by the entry launch behind the fast kernel, as before.  Nothing waits for anything that is not already submitted.
__device__ __forceinline__ void grx_lane_progress(const GrxLane& L) { if (L.progress && threadIdx.x == 0) atomicAdd(L.progress, 1); }   // fast kernel: this workgroup has ended
// entry launch (list == the step's entry list): 1 = entry e was taken by a polling workgroup
__device__ __forceinline__ int grx_lane_taken(const GrxLane& L, int e) {
  if (!L.ready || L.poll_grid != 0 || e >= L.ready_cap) return 0;
  int r = 0;
  if (threadIdx.x == 0) r = atomicCAS(L.ready + e, 1, 2) != 1;
  return __builtin_amdgcn_readfirstlane(r);
}
// polling workgroup p of the standing launch: the world to step, or -1
__device__ __forceinline__ int grx_lane_poll(const GrxLane& L, int p) {
  if (!L.ready || p >= L.ready_cap) return -1;
  int w = -1;
  if (threadIdx.x == 0) {
    for (int it = 0; it < 40000; it++) {      // bounded: ~40000 x 2 us
      int r = __hip_atomic_load(L.ready + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r == 0 && __hip_atomic_load(L.progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= L.progress_total)
        r = __hip_atomic_load(L.ready + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the fast launch has ended: one last look
      else if (r == 0) { __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); continue; }
      if (r == 1 && atomicCAS(L.ready + p, 1, 2) == 1) { __threadfence(); w = ((volatile const int*)L.poll_list)[p]; }
      break;
    }
  }
  return __builtin_amdgcn_readfirstlane(w);
}
// the body of a large-table kernel of the lane: a small fixed grid, one workgroup per entry of the compacted list (the caller sizes the grid: grx_overflow_lane.grid >= the
// list's cap) plus the polling workgroups behind them.  step(w): the family's step of one world, in_lane.  (Fetch's lane kernel keeps its own body: its entries carry a flag
// bit; Adroit's has the same body written out.)
template <class STEP>
__device__ __forceinline__ void grx_lane_walk(const GrxLane& L, STEP step) {
  const int e = blockIdx.x, nstand = (int)gridDim.x - L.poll_grid;
  if (e >= nstand) { const int w = grx_lane_poll(L, e - nstand); if (w >= 0) step(w); return; }
  if (e >= *L.count || grx_lane_taken(L, e)) return;
  step(L.list[e]);
}

// ---- state rows: qpos | qvel | warm start, the whole state of a world at a substep boundary.  Each row is given as base + offset in floats, so that the address is formed
// as the caller would form it itself: (b.qpos, (size_t)w * nq) is world w's row of a state buffer, (row, nq) the qvel part of a carrier row.  P: `float*`, or a volatile
// pointer for the two ends of a split step's hand-off (below).
template <class P, class O>
__device__ __forceinline__ void grx_state_load(GrxCtx& c, P qpos, O oq, P qvel, O ov, P qacc, O oa, int nq, int nv, int lane_) {
  for (int i = lane_; i < nq; i += 64) c.qpos[i] = qpos[oq + i];
  for (int i = lane_; i < nv; i += 64) { c.qvel[i] = qvel[ov + i]; c.qacc_ws[i] = qacc[oa + i]; }
}
template <class P, class O>
__device__ __forceinline__ void grx_state_store(const GrxCtx& c, P qpos, O oq, P qvel, O ov, P qacc, O oa, int nq, int nv, int lane_) {
  for (int i = lane_; i < nq; i += 64) qpos[oq + i] = c.qpos[i];
  for (int i = lane_; i < nv; i += 64) { qvel[ov + i] = c.qvel[i]; qacc[oa + i] = c.qacc_ws[i]; }
}

// ---- SPLIT STEP (include/grx_capi.h, grx_*_buffers.split_parts): `parts` workgroups per world, part p running the substeps [p T / parts, (p + 1) T / parts) of the slot's
// world; 0 of 1 = the whole step.  Part p + 1 was dispatched behind part p on the same XCD, so p is running or done when p + 1 starts.  Per world the launch has `split_state`
// words -- st[0]: the number of parts that have published (-1: an earlier part booked the world's re-run on the large tables), st[1]: the status flags of their substeps,
// st[2]: their measured time -- and a carrier row for the state (hand, Adroit, Kitchen: split_rows; Point: the world's own state rows, 2 words and no time; Fetch: its hand-off
// row, which also carries the flags, time in st[1]).
// How a part hands the world to the next one (MI355X_MICROARCH.md, workgroup dispatch / hand-off forms): the carrier row is written with write-through (volatile = sc0 sc1)
// stores, drained with s_waitcnt vmcnt(0), then the flag word is stored the same way; the reader polls the flag and reads the row with L1-bypassing (volatile) loads.  Valid for any
// workgroup -> XCD placement, and without an agent-scope release: `__threadfence()` writes back EVERY dirty line of the XCD's L2 (buffer_wbl2) -- the scratch of all resident waves --
// once per part and wave: that was 19 MB of write-back per launch of 4 096 worlds (PMC traffic 3.9x -> 10.6x algorithmic) and what made a third and fourth part cost more than they
// saved.  -DGRX_SPLIT_AGENT_FENCES restores the fences (A/B: tools/ab_split_fences.sh).
#ifdef GRX_SPLIT_AGENT_FENCES
#define GRX_SPLIT_ROW float
#define GRX_SPLIT_DRAIN() __threadfence()
#define GRX_SPLIT_ACQUIRE() __threadfence()
#else
#define GRX_SPLIT_ROW volatile float
#define GRX_SPLIT_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define GRX_SPLIT_ACQUIRE() asm volatile("" ::: "memory")
#endif
#define GRX_SPLIT_SPIN_LIMIT (1 << 22)   // polls (~64 cycles each: > 100 ms) before a part gives its predecessor up: never reached while workgroups of an XCD start in index order
// part > 0, before anything else: wait for the part before this one.  false = nothing to do here: the earlier part booked the world's re-run (v < 0; no part of a Point step
// ever does), or never came (v < part: flagged as a bad number); the last part then leaves the world's NW state words clean (Fetch 1, Point 2, hand / Adroit / Kitchen 3)
template <int NW>
__device__ __forceinline__ bool grx_split_wait(volatile int* st, int* status, int w, int part, bool last_part, int lane_) {
  int v = 0;
  for (int spins = 0; spins < GRX_SPLIT_SPIN_LIMIT; spins++) {
    v = __builtin_amdgcn_readfirstlane(st[0]);
    if (v == part || v < 0) break;
    __builtin_amdgcn_s_sleep(8);
  }
  if (v != part) {
    if (lane_ == 0) { if (v >= 0) status[w] |= GRX_ST_BADNUM | (GRX_ST_BADNUM << 16); if (last_part) for (int k = 0; k < NW; k++) st[k] = 0; }
    return false;
  }
  GRX_SPLIT_ACQUIRE();
  return true;
}
// the measured duration of a world, parked in its cost slot: the start stamp (device-wide 100 MHz clock) goes into the slot itself, so nothing stays live across the substep
// loop; the stop replaces it by the time since then in 80 ns units, plus what the earlier parts of a split step measured.  Lane 0 only.
__device__ __forceinline__ void grx_cost_start(int* cost, int w, int lane_) { if (cost && lane_ == 0) cost[w] = (int)wall_clock64(); }
__device__ __forceinline__ int grx_cost_since(const int* cost, int w) { const int t0 = ((volatile const int*)cost)[w]; return ((int)wall_clock64() - t0) >> 3; }
__device__ __forceinline__ void grx_cost_stop(int* cost, int w, int earlier) { cost[w] = grx_cost_since(cost, w) + earlier; }
// An earlier part, after its substeps, publishes: the state goes to the carrier row, GRX_SPLIT_DRAIN, barrier, then lane 0 books what the part adds to the state words,
// GRX_SPLIT_DRAIN, st[0] = part + 1.  Nothing else is written.  This stays written out in each family (as a helper it moved the register allocation of the hand and Kitchen
// kernels, profiles/kernel_resources_step_frame.txt); the differences between the five copies are these, and all are intended:
//   overflow   a part whose world exceeded a table books st[0] = -1 and stores nothing (the re-run on the large tables is booked: the later parts return): Fetch, hand, Adroit,
//              Kitchen.  Point has no overflow lane and no such branch.
//   barrier    in front of the row store, so that it comes behind every lane's last LDS write of the simulation: Point, Adroit and Kitchen have it inside the publish; the hand's
//              is the barrier behind its simulation call, just above; Fetch has none (a workgroup is one wavefront, whose LDS accesses complete in order: the barrier is the
//              conservative form, not a requirement).
//   row        hand, Adroit, Kitchen: split_rows, qpos | qvel | warm start.  Point: the world's own state rows.  Fetch: the hand-off row, [0] resume substep, [1] the flags of the
//              substeps so far, then ctrl | mocap | qpos | qvel | warm start, plus the hull cache row.
//   words      hand, Adroit, Kitchen: flags OR-ed into st[1], time added to st[2] where the launch is timed.  Point: flags into st[1], no time.  Fetch: flags travel in the row,
//              time is added to st[1].
// the last part, after its substeps: the flags of the earlier parts join its own, their measured time is returned (NW == 3), and the words are clean for the next launch
template <int NW>
__device__ __forceinline__ int grx_split_collect(GrxCtx& c, volatile int* st, int lane_) {
  int earlier = 0;
  if (lane_ == 0) { c.cnt[2] |= st[1]; if (NW > 2) earlier = st[2]; for (int k = 0; k < NW; k++) st[k] = 0; }
  __syncthreads();
  return earlier;
}

// ---- stage profile (-DGRX_PROFILE): the prologue behind grx_ctx_carve and the epilogue of every kernel that runs the engine; g_grx_prof is summed over worlds
#ifdef GRX_PROFILE
#define GRX_PROF_BEGIN(c, lane_) \
  __shared__ long long prof_s[GRX_NPROF + 1]; \
  (c).prof = prof_s; (c).prof_last = prof_s + GRX_NPROF; \
  if ((lane_) == 0) { for (int k = 0; k < GRX_NPROF; k++) prof_s[k] = 0; prof_s[GRX_NPROF] = clock64(); }
#define GRX_PROF_END(c, lane_) do { \
  GRX_TICK(&(c), GRX_P_OTHER); \
  if ((lane_) == 0) for (int k = 0; k < GRX_NPROF; k++) atomicAdd((unsigned long long*)&g_grx_prof[k], (unsigned long long)(c).prof[k]); } while (0)
#else
#define GRX_PROF_BEGIN(c, lane_)
#define GRX_PROF_END(c, lane_) ((void)0)
#endif
