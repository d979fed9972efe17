/* maze_rollout.c -- an AntMaze rollout through the env-level C ABI alone (include/grx_env.h): the maze twin of fetch_rollout.c.
 *
 *     python -m gymnasium_robotics_amd.env_capi describe AntMaze_UMaze-v5 ant.grxenv
 *     cc -std=c99 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include tests/capi/maze_rollout.c \
 *        -L gymnasium_robotics_amd/_lib -lgrx_env -lgrx_hip -L /opt/rocm/lib -lamdhip64 -Wl,-rpath,gymnasium_robotics_amd/_lib -o maze_rollout
 *     ./maze_rollout ant.grxenv 64 60
 *
 * N worlds, world i seeded with 1000 + i, same-step autoreset with a horizon of 20 steps (three episodes per world in 60 steps),
 * deterministic actions.  The flags and the list of finished worlds are decided on the device: grx_env_outputs waits for their copy
 * only.  Prints the number of finished episodes and an FNV-1a checksum of the packed rows after the last step
 * (tests/test_gpu_env_capi_maze.py compares it with the same rollout driven through ctypes). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "grx_env.h"

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
  grx_env_config cfg = {GRX_ENV_SAME_STEP, 20, 0};
  grx_env* env = NULL;
  CHECK(grx_env_create(argv[1], n, 0, &cfg, &env));
  int obs_dim, goal_dim, act_dim;
  double dt;
  CHECK(grx_env_dims(env, &obs_dim, &goal_dim, &act_dim, &dt));
  uint64_t* seeds = malloc(sizeof(uint64_t) * n);
  float* packed = malloc(sizeof(float) * n * (obs_dim + 2 * goal_dim + 2));
  float* actions = NULL;      /* pinned: grx_env_step copies it on the stream, without waiting */
  if (!seeds || !packed || hipHostMalloc((void**)&actions, sizeof(float) * n * act_dim, 0) != hipSuccess) return 1;
  for (int i = 0; i < n; ++i) seeds[i] = 1000 + (uint64_t)i;
  CHECK(grx_env_reset(env, NULL, seeds, NULL));
  long finished = 0;
  for (int t = 0; t < steps; ++t) {
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < act_dim; ++j) actions[i * act_dim + j] = action_value(t, i, j);
    CHECK(grx_env_step(env, actions, NULL));
    grx_env_device_outputs out;
    CHECK(grx_env_outputs(env, &out));      /* device rows for a policy on the GPU; flags and the finished worlds on the host (waits for their copy) */
    finished += out.n_final;
    if (hipStreamSynchronize(NULL) != hipSuccess) return 1;      /* before the pinned actions are rewritten */
  }
  grx_env_host_outputs host = {0};
  host.packed = packed;
  CHECK(grx_env_copy_outputs(env, &host));
  uint64_t h = 1469598103934665603ull;      /* FNV-1a 64 over the bytes of the packed rows */
  const unsigned char* p = (const unsigned char*)packed;
  for (size_t k = 0; k < sizeof(float) * (size_t)n * (obs_dim + 2 * goal_dim + 2); ++k) h = (h ^ p[k]) * 1099511628211ull;
  printf("finished %ld\nchecksum %016llx\n", finished, (unsigned long long)h);
  CHECK(grx_env_destroy(env));
  (void)hipHostFree(actions);
  free(seeds);
  free(packed);
  return 0;
}
