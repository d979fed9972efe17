/* grx_episodes.h -- an on-device store of FINISHED episodes with hindsight sampling, attached to a replay of the env-level C ABI (grx_replay.h), implemented in
 * libgrx_env.so.
 *
 * The replay of grx_replay.h draws from the episodes that are still running: a transition can be relabelled only while its episode is in the ring.  The store keeps the
 * episodes that have ENDED -- gymnasium_robotics_amd/her.py (EpisodicHerReplay) for a caller that is not Python -- in device memory, episode-major:
 *     rows  [episodes, horizon + 1, packed_width]   the packed rows of the episode, row 0 first
 *     acts  [episodes, horizon + 1, act_dim]        acts[e, j] = the action that led to row j (row 0: zero)
 *     meta  [episodes, 4] int32                     {len, world, first_row, 0}: len = the number of transitions, 0 = empty slot
 *     count [1] int64                               episodes archived so far; slot = count % episodes, the oldest episode is overwritten
 * and grx_episodes_sample draws relabelled transitions from whole episodes in the row format of grx_replay_relabel: "future" goals from the whole rest of the episode,
 * the "final" and "episode" strategies, and a fresh relabel of old experience at every call (the buffer of Andrychowicz et al. 2017).
 *
 * With a store attached, grx_replay_append first moves the episodes of the worlds that step ended into the store (two small launches), then appends as before.  The
 * order matters and is the library's business: the archive must see the ring before this step's row overwrites the oldest one, and the episode marks before the reset
 * worlds are re-marked.  With keep_final in same-step mode a stored episode ends with the terminal row and the action that led to it; otherwise with the newest ring row
 * (same-step without keep_final: the last transition is not stored, as in the ring).  An episode longer than the horizon keeps its last `horizon` transitions.
 * The ring, the marks and every grx_replay_relabel batch are bit for bit what they are without a store.
 *
 * No call waits for the device or reads device memory: the list of ended worlds is the one the step left on the device (its length a device word for a maze handle with
 * device-side bookkeeping), count lives on the device, and "is there anything to sample" is answered by the sampling kernel.
 *
 * Order of calls: grx_replay_create -> grx_episodes_create (one store per replay) -> ... -> grx_episodes_destroy -> grx_replay_destroy (which refuses while a store is
 * attached).  grx_replay_begin keeps the store.  The store is not part of the handle's state blob.  Every call returns 0 or GRX_ENV_EINVAL / GRX_ENV_EHIP and leaves its
 * message for the last-error call of grx_env.h.
 */
#ifndef GRX_EPISODES_H
#define GRX_EPISODES_H

#include <stddef.h>
#include <stdint.h>

#include "grx_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grx_episodes grx_episodes;

enum { GRX_EPISODES_FUTURE = 0, GRX_EPISODES_FINAL = 1, GRX_EPISODES_EPISODE = 2 };

typedef struct grx_episodes_config {
  int64_t episodes;    /* slots, >= the handle's number of worlds (one step can end an episode in every world) and < 2^31 */
  int64_t max_batch;   /* the largest batch sample will be asked for, >= 1 */
  uint64_t seed;       /* index stream of sample; independent of the replay's */
} grx_episodes_config;

typedef struct grx_episodes_batch {
  const float* rows;       /* device [batch, row_width]: the store's own buffer, overwritten by the next sample */
  int64_t batch;
  const int32_t* valid;    /* device [1]: batch, or 0 when the store holds no episode (rows zero-filled) */
} grx_episodes_batch;

/* Allocates the store (zero-filled) on the handle's device and attaches it to the replay.  EINVAL: NULL argument, episodes < number of worlds or >= 2^31, max_batch < 1,
 * a store already attached. */
int grx_episodes_create(grx_replay* replay, const grx_episodes_config* cfg, grx_episodes** out);
/* Detaches and frees (synchronises the device). */
int grx_episodes_destroy(grx_episodes* eps);
int grx_episodes_dims(const grx_episodes* eps, int* row_width, int* horizon, int* packed_width, int* act_dim);
/* Draws `batch` transitions from the stored episodes and writes them, relabelled, into the store's batch buffer: a uniform stored episode, a uniform transition t of it,
 * and with probability k_future / (k_future + 1) a substituted goal -- FUTURE: achieved at a uniform later row, FINAL: at the episode's last row, EPISODE: at a uniform
 * row of the episode; reward and success recomputed.  One kernel; the counter-based stream of grx_her_episode_sample (grx_capi.h): seed, call counter, sample index.
 * The call counter advances on every call.  EINVAL: batch < 1, batch > max_batch, k_future < 0, unknown strategy. */
int grx_episodes_sample(grx_episodes* eps, int64_t batch, int k_future, int strategy, grx_episodes_batch* out, void* stream);
/* Restarts the index stream: the same (seed, number of sample calls since) reproduces the same draws. */
int grx_episodes_reseed(grx_episodes* eps, uint64_t seed);
/* The store's device arrays (layout above) and its number of slots, for inspection or a learner's own kernels. */
int grx_episodes_store(const grx_episodes* eps, const float** rows, const float** acts, const int32_t** meta, const int64_t** count_dev, int64_t* episodes);

#ifdef __cplusplus
}
#endif
#endif
