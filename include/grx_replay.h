/* grx_replay.h -- on-device hindsight experience replay (HER) for a handle of the env-level C ABI (grx_env.h), implemented in libgrx_env.so.
 *
 * The storage and relabelling of gymnasium_robotics_amd/her.py (HerReplay(env, horizon, capacity, seed, continuous=True)) for a caller that is not Python, attached to a
 * handle of either family: a ring of the last horizon + 1 packed rows of every world and the actions that led to them, the episode boundaries of every world, and a replay
 * ring of relabelled transitions
 *     [obs_t | achieved_t | goal | action_t | reward | obs_t+1 | achieved_t+1 | success]          row_width = 2 obs_dim + 3 goal_dim + act_dim + 2
 * all in device memory.  The reward parameters are the ones the handle was described with (Fetch: the task's distance threshold; maze: the goal radius; sparse or dense),
 * the values the batched reward call of grx_env.h uses.
 *
 * Nothing here keeps a host mirror of the episodes.  The worlds a step reset are taken from the list that step already left on the device -- for a maze handle with
 * device-side bookkeeping a list whose LENGTH is a device word -- and whether anything can be sampled is decided by the sampling kernel.  So append and relabel enqueue
 * and return: neither waits for the device nor reads device memory, for either handle kind in any mode.  append is one kernel, relabel two.
 *
 * Order of calls: create (after the handle; one replay per handle) -> [reset or set_state of the handle -> begin -> (step of the handle -> append -> relabel ...)] ->
 * destroy (before the handle is destroyed).  Every call returns 0 or GRX_ENV_EINVAL / GRX_ENV_EHIP and leaves its message for the last-error call of grx_env.h;
 * "stream" is a hipStream_t (NULL = the null stream) and must be the stream the handle is stepped on.
 *
 * Two documented differences from HerReplay: when no world has a transition to sample (every world was reset in the step just appended) relabel still takes its slot --
 * zero-filled, valid[0] = 0 -- and the head and the call counter of the index stream advance, where HerReplay.relabel returns an empty view and advances neither.
 * Checkpointing the replay contents is out of scope: the state blob of the handle does not hold them; after a restore, call begin and refill.
 */
#ifndef GRX_REPLAY_H
#define GRX_REPLAY_H

#include <stddef.h>
#include <stdint.h>

#include "grx_env.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grx_replay grx_replay;

typedef struct grx_replay_config {
  int horizon;         /* T >= 1: the episode ring keeps the last T + 1 rows of every world (a transition older than T steps is no longer sampled) */
  int keep_final;      /* same-step autoreset only: keep the finished episode's last transition sampleable in the step that ends it, its next observation being the terminal
                        * row (HerReplay.append(final_rows=...)); ignored in the other autoreset modes */
  int64_t capacity;    /* rows of the replay ring, >= 1 */
  int64_t max_batch;   /* the largest batch relabel will be asked for (relabel refuses larger ones); <= 0: capacity */
  uint64_t seed;       /* index stream, as HerReplay(seed=...) */
} grx_replay_config;

typedef struct grx_replay_batch {
  const float* rows;       /* device [batch, row_width]: the slot of the replay ring just written */
  int64_t batch, offset;   /* offset: first row of the slot inside the ring */
  const int32_t* valid;    /* device [1]: batch, or 0 when no world had a transition to sample (the slot is zero-filled); overwritten by the next relabel */
} grx_replay_batch;

/* Allocates the rings (zero-filled) on the handle's device and attaches the replay to the handle.  EINVAL: NULL argument, horizon < 1, capacity < 1,
 * max_batch > capacity, a replay already attached. */
int grx_replay_create(grx_env* env, const grx_replay_config* cfg, grx_replay** out);
/* Detaches and frees (synchronises the device). */
int grx_replay_destroy(grx_replay* r);
int grx_replay_dims(const grx_replay* r, int* row_width, int* obs_dim, int* goal_dim, int* act_dim);
/* After a reset / set_state of the handle, on the same stream: ring row 0 <- the handle's current packed rows, row counter 0, and episode_start[w] = -elapsed[w] from the
 * handle's own time-limit counters (a host vector, or the device array of a maze handle with device-side bookkeeping), so a staggered batch -- a restored state -- is
 * sampled correctly from the first step: HerReplay.begin_episode followed by set_episode_start(-elapsed).  The replay ring, its head and the index stream are kept. */
int grx_replay_begin(grx_replay* r, void* stream);
/* After each step of the handle, same stream: row t + 1 <- the packed rows and the actions of that step (the handle's own action buffer: no action pointer), and the
 * worlds whose row is the first of a new episode are marked (same-step autoreset: the worlds the step finished and reset; next-step: the worlds it reset in place of
 * stepping them).  With keep_final the terminal rows of a maze handle are scattered into a per-world buffer of the replay (a Fetch handle keeps them per world already).
 * ONE kernel, no copy.  EINVAL: before begin; twice without a step between; a step that was not appended; a reset / set_state of the handle since begin. */
int grx_replay_append(grx_replay* r, void* stream);
/* Draws `batch` transitions ("future" strategy, k_future / (k_future + 1) of them with a goal achieved later in the same episode; the counter-based stream of
 * grx_her_sample_final, grx_capi.h: seed, call counter, sample index), relabels them and writes one contiguous slot at the head of the replay ring (the head wraps to 0
 * when the slot would not fit).  Two kernels.  EINVAL: batch < 1, batch > max_batch, k_future < 0. */
int grx_replay_relabel(grx_replay* r, int64_t batch, int k_future, grx_replay_batch* out, void* stream);
/* Restarts the index stream: the same (seed, number of relabel calls since) reproduces the same draws. */
int grx_replay_reseed(grx_replay* r, uint64_t seed);
/* The replay ring: device [capacity, row_width]; head = the row the next slot starts at (before wrapping), size = rows written so far (at most capacity).  Host values. */
int grx_replay_ring(const grx_replay* r, const float** rows, int64_t* capacity, int64_t* head, int64_t* size);

#ifdef __cplusplus
}
#endif
#endif
