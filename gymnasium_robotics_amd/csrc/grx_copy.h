// grx_copy.h -- the flat row copy shared by the HER append kernel (grx_kernels.hip) and the replay's begin kernel (grx_env_replay.inc)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// flat copy of n words by the whole grid: 16-byte accesses when both bases allow (an environment's rows always do; a ring row does unless N W is odd), the tail word by word
static __device__ __forceinline__ void grx_copy_words(float* __restrict__ dst, const float* __restrict__ src, long long n, long long tid, long long nth) {
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
    const long long n4 = n >> 2;
    const float4* __restrict__ s4 = (const float4*)src;
    float4* __restrict__ d4 = (float4*)dst;
    for (long long i = tid; i < n4; i += nth) d4[i] = s4[i];
    for (long long i = (n4 << 2) + tid; i < n; i += nth) dst[i] = src[i];
  } else {
    for (long long i = tid; i < n; i += nth) dst[i] = src[i];
  }
}
