/* grx_norm.h -- on-device observation and goal normaliser for HER batches, attached to a handle of the env-level C ABI (grx_env.h), implemented in libgrx_env.so.
 *
 * What every DDPG + HER learner does to the rows of grx_replay.h / grx_episodes.h (Andrychowicz et al. 2017; Plappert et al. 2018): keep running per-component mean and
 * standard deviation of observations and goals, update them from the relabelled transitions, and feed the networks (x - mean) / std clipped to +-clip.  The statistics
 * live in device memory -- D = obs_dim + goal_dim columns, the observation columns first:
 *     sum[D] f64, sumsq[D] f64, count[1] i64, skipped[1] i64, mean[D] f32, inv_std[D] f32
 * Of a replay row [obs_t | achieved_t | goal | action_t | reward | obs_t+1 | achieved_t+1 | success] update tracks obs_t and the relabelled goal (the published recipe).
 * The arithmetic is that of the grx_normstat calls of grx_capi.h, which these calls issue: fp64 sums without floating-point atomics in a fixed order (bit-identical from
 * run to run), a row with a non-finite tracked value skipped and counted, the refresh mean = sum / count, std = sqrt(max(eps^2, sumsq / count - mean^2)) in fp64, and
 * y = min(max((x - mean) * inv_std, -clip), clip) in fp32 in that order, a NaN staying a NaN.
 *
 * No call waits for the device or reads device memory except where it says "synchronises".  update takes the `rows` and `valid` fields of a grx_replay_batch or a
 * grx_episodes_batch as they are: whether the slot holds anything (valid[0]) is read by the kernels.
 *
 * Order of calls: create (after the handle; one normaliser per handle) -> per learner step: grx_replay_relabel / grx_episodes_sample -> update -> apply_batch, and
 * policy_input before the actor chooses the next action -> destroy (before the handle is destroyed: grx_env_destroy refuses while a normaliser is attached).  Every call
 * returns 0 or GRX_ENV_EINVAL / GRX_ENV_EHIP and leaves its message for the last-error call of grx_env.h; "stream" is a hipStream_t (NULL = the null stream), the stream
 * the rows were written on.
 *
 * Unlike the replay contents the statistics are checkpointable: they are a few hundred bytes and a resumed run is wrong without them.  The state blob (host memory,
 * little endian): magic[8] "GRXNORM\0", u32 version (1), i32 obs_dim, i32 goal_dim, u32 0, f64 eps, f32 clip, u32 0, then sum[D] f64, sumsq[D] f64, i64 count, i64 skipped.
 */
#ifndef GRX_NORM_H
#define GRX_NORM_H

#include <stddef.h>
#include <stdint.h>

#include "grx_env.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grx_norm grx_norm;

typedef struct grx_norm_config {
  double eps;      /* floor of the standard deviation, > 0 */
  float clip;      /* normalised values are clipped to [-clip, clip], > 0 */
} grx_norm_config;

/* Allocates the statistics (zero: count 0, mean 0, inv_std 1) on the handle's device and attaches the normaliser; the dimensions are the handle's.  cfg NULL: eps 1e-2,
 * clip 5.  EINVAL: NULL handle or out, eps <= 0, clip <= 0, a normaliser already attached. */
int grx_norm_create(grx_env* env, const grx_norm_config* cfg, grx_norm** out);
/* Detaches and frees (synchronises). */
int grx_norm_destroy(grx_norm* norm);
int grx_norm_dims(const grx_norm* norm, int* row_width, int* obs_dim, int* goal_dim, int* act_dim);
/* Adds `batch` replay rows (device [batch, row_width]) to the statistics and refreshes mean / inv_std: two launches.  valid: device int32[1] or NULL; valid[0] == 0: nothing
 * changes. */
int grx_norm_update(grx_norm* norm, const float* rows, int64_t batch, const int32_t* valid, void* stream);
/* out [batch, row_width] <- rows with obs_t, obs_t+1 (observation statistics) and achieved_t, goal, achieved_t+1 (goal statistics) normalised and clipped, action / reward /
 * success copied.  out == rows is allowed.  One launch. */
int grx_norm_apply_batch(grx_norm* norm, const float* rows, int64_t batch, float* out, void* stream);
/* The actor's input for the step about to be taken: the handle's current packed rows -> *out, device [num_envs, obs_dim + goal_dim] = [norm(obs) | norm(desired)], a buffer
 * the normaliser owns; valid until the next call of this function.  One launch. */
int grx_norm_policy_input(grx_norm* norm, const float** out, void* stream);
/* Device pointers of the statistics (any may be NULL); *dim = obs_dim + goal_dim. */
int grx_norm_stats(const grx_norm* norm, const float** mean, const float** inv_std, const double** sum, const double** sumsq, const int64_t** count, const int64_t** skipped,
                   int* dim);
/* The state blob (layout above).  get and set synchronise.  set refuses a blob of other dimensions (EINVAL), takes eps and clip from the blob, and recomputes mean and
 * inv_std on the device with the refresh code of update. */
int grx_norm_state_size(const grx_norm* norm, size_t* bytes);
int grx_norm_get_state(grx_norm* norm, void* blob, size_t bytes);
int grx_norm_set_state(grx_norm* norm, const void* blob, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
