/* episodes_rollout.c -- a Fetch rollout whose finished episodes are kept in an on-device store and sampled with hindsight goals, through the C ABI alone
 * (include/grx_env.h, include/grx_replay.h, include/grx_episodes.h): INTEGRATION.md section 1e.
 *
 *     python -m gymnasium_robotics_amd.env_capi describe FetchPickAndPlace-v4 pick.grxenv
 *     cc -std=c99 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include tests/capi/episodes_rollout.c \
 *        -L gymnasium_robotics_amd/_lib -lgrx_env -lgrx_hip -L /opt/rocm/lib -lamdhip64 -Wl,-rpath,gymnasium_robotics_amd/_lib -o episodes_rollout
 *     ./episodes_rollout pick.grxenv 64 60
 *
 * N worlds, world i seeded with 1000 + i, same-step autoreset with a horizon of 25 steps, deterministic actions.  Every step is appended to the replay (horizon 25, the
 * terminal rows kept); the append first moves the episodes that step ended into a store of 2 N slots.  After every step 4 N transitions are drawn from the stored episodes,
 * the strategy changing with the step (future, final, episode).  Nothing in the loop reads device memory; the one synchronise per step only protects the pinned action
 * buffer.  Prints the row width, the `valid` word of the last batch and an FNV-1a checksum of its rows (tests/test_gpu_episode_replay.py compares it with the same rollout
 * driven through ctypes). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "grx_env.h"
#include "grx_episodes.h"
#include "grx_replay.h"

#define CHECK(call)                                                                          \
  do {                                                                                       \
    int rc_ = (call);                                                                        \
    if (rc_ != 0) {                                                                          \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, grx_env_last_error());             \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

/* action j of world i at step t: multiples of 1/8 in [-1, 1) */
static float action_value(int t, int i, int j) { return (float)((t * 11 + i * 7 + j * 3) % 17) / 8.0f - 1.0f; }

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <description file> [num_envs] [steps]\n", argv[0]);
    return 2;
  }
  const int n = argc > 2 ? atoi(argv[2]) : 64, steps = argc > 3 ? atoi(argv[3]) : 60;
  grx_env_config cfg = {GRX_ENV_SAME_STEP, 25, 0};
  grx_env* env = NULL;
  CHECK(grx_env_create(argv[1], n, 0, &cfg, &env));
  int obs_dim, goal_dim, act_dim, row_width;
  double dt;
  CHECK(grx_env_dims(env, &obs_dim, &goal_dim, &act_dim, &dt));
  const int64_t batch = 4 * (int64_t)n;
  grx_replay_config rcfg = {25, 1, 16 * batch, batch, 5};      /* horizon, keep_final, capacity, max_batch, seed */
  grx_replay* replay = NULL;
  CHECK(grx_replay_create(env, &rcfg, &replay));
  grx_episodes_config ecfg = {2 * (int64_t)n, batch, 9};       /* episodes, max_batch, seed */
  grx_episodes* store = NULL;
  CHECK(grx_episodes_create(replay, &ecfg, &store));
  CHECK(grx_episodes_dims(store, &row_width, NULL, NULL, NULL));
  uint64_t* seeds = malloc(sizeof(uint64_t) * n);
  float* rows = malloc(sizeof(float) * (size_t)batch * row_width);
  float* actions = NULL;      /* pinned: grx_env_step copies it on the stream, without waiting */
  if (!seeds || !rows || hipHostMalloc((void**)&actions, sizeof(float) * n * act_dim, 0) != hipSuccess) return 1;
  for (int i = 0; i < n; ++i) seeds[i] = 1000 + (uint64_t)i;
  CHECK(grx_env_reset(env, NULL, seeds, NULL));
  CHECK(grx_replay_begin(replay, NULL));
  grx_episodes_batch last = {0};
  for (int t = 0; t < steps; ++t) {
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < act_dim; ++j) actions[i * act_dim + j] = action_value(t, i, j);
    CHECK(grx_env_step(env, actions, NULL));
    CHECK(grx_replay_append(replay, NULL));      /* archives the episodes this step ended, then appends */
    CHECK(grx_episodes_sample(store, batch, 4, t % 3, &last, NULL));      /* a learner on the GPU reads last.rows behind this, on the same stream */
    if (hipStreamSynchronize(NULL) != hipSuccess) return 1;      /* before the pinned actions are rewritten */
  }
  int32_t valid = -1;
  if (hipMemcpy(rows, last.rows, sizeof(float) * (size_t)batch * row_width, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (hipMemcpy(&valid, last.valid, sizeof valid, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  uint64_t h = 1469598103934665603ull;      /* FNV-1a 64 over the bytes of the last batch */
  const unsigned char* p = (const unsigned char*)rows;
  for (size_t k = 0; k < sizeof(float) * (size_t)batch * row_width; ++k) h = (h ^ p[k]) * 1099511628211ull;
  printf("row_width %d\nvalid %d\nchecksum %016llx\n", row_width, (int)valid, (unsigned long long)h);
  CHECK(grx_episodes_destroy(store));
  CHECK(grx_replay_destroy(replay));
  CHECK(grx_env_destroy(env));
  (void)hipHostFree(actions);
  free(seeds);
  free(rows);
  return 0;
}
