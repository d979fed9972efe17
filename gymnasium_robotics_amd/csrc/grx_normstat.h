// grx_normstat.h -- running observation / goal statistics of HER batches and their application (include/grx_capi.h, grx_normstat_*), included by the API unit of grx_kernels.hip.
//
// A stat block for (obs_dim, goal_dim), D = obs_dim + goal_dim columns, is one device allocation (byte offsets: grx_normstat_layout):
//     sum[D] f64 | sumsq[D] f64 | count i64 | skipped i64 | mean[D] f32 | inv_std[D] f32 | (pad to 16) | partial[kNormGroups][2 D] f64 | pskip[kNormGroups] i64
// The last two arrays are the update's workspace.  An update is two launches: workgroup g of the first sums the row chunks g, g + G, g + 2 G, ... (kNormRows rows each)
// in ascending order into partial[g], the single workgroup of the second adds the partials in a fixed order to the running sums and refreshes mean / inv_std.  The launch
// boundary is the hand-off, so there is no in-launch fence or ticket, and there is no floating-point atomic: the same rows and the same prior block give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int kNormRows = 64;          // rows per chunk (grx_normstat_geometry)
constexpr int kNormGroups = 1024;      // workgroups of the update launch at most
constexpr int kNormTile = 8192;        // words of one staged tile: row_width <= kNormTile
constexpr int kNormMaxD = 256;         // one thread per tracked column
constexpr int kNormMaxWidth = 4096;    // apply_batch: the per-column table in LDS (8 bytes per column)

struct GrxNormLayout {
  long long sum, sumsq, count, skipped, mean, inv_std, public_bytes, partial, pskip, total_bytes;
};

static inline GrxNormLayout grx_norm_layout(int D) {
  GrxNormLayout L;
  L.sum = 0; L.sumsq = 8ll * D; L.count = 16ll * D; L.skipped = L.count + 8; L.mean = L.skipped + 8; L.inv_std = L.mean + 4ll * D; L.public_bytes = L.inv_std + 4ll * D;
  L.partial = (L.public_bytes + 15) / 16 * 16;
  L.pskip = L.partial + 16ll * D * kNormGroups;
  L.total_bytes = L.pskip + 8ll * kNormGroups;
  return L;
}

static __device__ __forceinline__ bool grx_norm_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// fp32, in this order: subtract, multiply, clip.  The compares are false for a NaN, which therefore stays; +-inf times a positive inv_std clips.
static __device__ __forceinline__ float grx_norm_one(float x, float m, float s, float clip) {
  float y = __fmul_rn(__fsub_rn(x, m), s);
  y = y < -clip ? -clip : y;
  y = y > clip ? clip : y;
  return y;
}

struct GrxNormUpdateArgs {
  const float* rows; long long batch; int W, od, gd;
  const int* valid;
  double* partial; long long* pskip;
};

extern "C" __global__ void __launch_bounds__(256)
grx_norm_update_kernel(GrxNormUpdateArgs a) {
  __shared__ __align__(16) float tile[kNormTile + 4];
  __shared__ int bad[kNormRows];
  __shared__ int nskip;
  if (a.valid && a.valid[0] == 0) return;      // the zero-filled slot of a relabel that had nothing to sample: decided here, not on the host
  const int t = threadIdx.x, W = a.W, D = a.od + a.gd;
  const int lanes = 256 / D, c = t % D, lane = t / D;
  const bool active = lane < lanes;
  const int col = c < a.od ? c : c + a.gd;      // the relabelled goal sits behind achieved_t
  const int sub = kNormTile / W < kNormRows ? kNormTile / W : kNormRows;
  if (t == 0) nskip = 0;
  double s = 0.0, q = 0.0;
  int skipped = 0;
  for (long long chunk = blockIdx.x; chunk * kNormRows < a.batch; chunk += gridDim.x) {
    const long long r0 = chunk * kNormRows;
    const int nr = a.batch - r0 < kNormRows ? (int)(a.batch - r0) : kNormRows;
    for (int t0 = 0; t0 < nr; t0 += sub) {
      const int m = nr - t0 < sub ? nr - t0 : sub;
      const float* src = a.rows + (size_t)(r0 + t0) * W;
      const int words = m * W;
      // rows start at any 4-byte boundary (odd widths): words up to the first 16-byte boundary one by one, then 16-byte loads; the tile is shifted so that both sides align
      const int pad = (int)(((uintptr_t)src >> 2) & 3);
      int head = (4 - pad) & 3;
      if (head > words) head = words;
      const int n4 = (words - head) >> 2;
      __syncthreads();      // the previous tile has been consumed
      if (t < head) tile[pad + t] = src[t];
      const float4* s4 = (const float4*)(src + head);
      float4* d4 = (float4*)(tile + pad + head);
#pragma unroll 4
      for (int i = t; i < n4; i += 256) d4[i] = s4[i];
      for (int i = head + (n4 << 2) + t; i < words; i += 256) tile[pad + i] = src[i];
      if (t < m) bad[t] = 0;
      __syncthreads();
      const float* tl = tile + pad;
      if (active)
        for (int r = lane; r < m; r += lanes)
          if (grx_norm_nonfinite(tl[r * W + col])) bad[r] = 1;      // every writer writes 1
      __syncthreads();
      if (active)
        for (int r = lane; r < m; r += lanes)
          if (!bad[r]) {
            const double x = (double)tl[r * W + col];
            s += x;
            q += x * x;      // exact in fp64
          }
      if (t < m && bad[t]) skipped += 1;
    }
  }
  __syncthreads();
  double* red = (double*)tile;      // [2][256]
  red[t] = s;
  red[256 + t] = q;
  if (skipped) atomicAdd(&nskip, skipped);
  __syncthreads();
  if (t < D) {
    double ts = 0.0, tq = 0.0;
    for (int l = 0; l < lanes; ++l) { ts += red[l * D + t]; tq += red[256 + l * D + t]; }
    double* p = a.partial + (size_t)blockIdx.x * 2 * D;
    p[t] = ts;
    p[D + t] = tq;
  }
  if (t == 0) a.pskip[blockIdx.x] = nskip;
}

// One workgroup: partials -> running sums (fixed order), counters, then mean / inv_std of every column in fp64.  ngroups == 0: refresh only (grx_normstat_refresh).
extern "C" __global__ void __launch_bounds__(256)
grx_norm_finish_kernel(double* sums, long long* count, long long* skipped, float* mean, float* inv_std, const double* partial, const long long* pskip, int ngroups,
                       long long batch, int D, const int* valid, double eps) {
  __shared__ double red[8][32];
  __shared__ unsigned long long sk_all;
  __shared__ long long cnt_now;
  if (valid && valid[0] == 0) return;
  const int t = threadIdx.x;
  if (t == 0) sk_all = 0ull;
  __syncthreads();
  if (ngroups > 0) {
    unsigned long long sk = 0ull;
    for (int g = t; g < ngroups; g += 256) sk += (unsigned long long)pskip[g];
    if (sk) atomicAdd(&sk_all, sk);
    const int j1 = t & 31, slice = t >> 5;
    for (int j0 = 0; j0 < 2 * D; j0 += 32) {
      const int j = j0 + j1;
      double acc = 0.0;
      for (int g0 = slice; g0 < ngroups; g0 += 8 * 16) {      // slice s adds the groups s, s + 8, s + 16, ... in that order; sixteen loads in flight, the adds behind them
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int g = g0 + 8 * k;
          v[k] = (j < 2 * D && g < ngroups) ? partial[(size_t)g * 2 * D + j] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) acc += v[k];
      }
      red[slice][j1] = acc;
      __syncthreads();
      if (t < 32 && j < 2 * D) {
        double tot = red[0][t];
        for (int k = 1; k < 8; ++k) tot += red[k][t];
        sums[j] += tot;      // sum[D] and sumsq[D] are contiguous
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (t == 0) {
    long long cn = count[0];
    if (ngroups > 0) {
      cn += batch - (long long)sk_all;
      count[0] = cn;
      skipped[0] += (long long)sk_all;
    }
    cnt_now = cn;
  }
  __syncthreads();
  const long long cn = cnt_now;
  for (int c = t; c < D; c += 256) {
    float m = 0.0f, is = 1.0f;
    if (cn > 0) {
      const double n = (double)cn;
      const double mu = sums[c] / n;
      double mu2 = mu * mu;
      asm volatile("" : "+v"(mu2));      // a rounded product of its own: contracted into the subtraction (one fma) the variance differs from the stated formula
      const double var = sums[D + c] / n - mu2;
      const double e2 = eps * eps;
      const double sd = sqrt(var > e2 ? var : e2);
      m = (float)mu;
      is = (float)(1.0 / sd);
    }
    mean[c] = m;
    inv_std[c] = is;
  }
}

// out[b, c] = normalised rows[b, c] for the observation and goal columns of a replay row, the other columns copied.  Flat over the words, 16 bytes per access where rows
// and out share their offset from a 16-byte boundary (always when in place); the column of a thread's next access advances by a fixed step, so there is no division
// in the loop.  No __restrict__: out == rows is allowed.
extern "C" __global__ void __launch_bounds__(256)
grx_norm_apply_batch_kernel(const float* mean, const float* inv_std, const float* rows, float* out, long long n, int W, int od, int gd, int ad, float clip) {
  extern __shared__ float2 grx_norm_tab[];      // per column: (mean, inv_std), inv_std == 0: copied through
  float2* tab = grx_norm_tab;
  const int t = threadIdx.x;
  for (int c = t; c < W; c += 256) {
    const int o2 = od + 2 * gd + ad + 1;      // obs_t+1
    int k = -1;
    if (c < od) k = c;
    else if (c < od + gd) k = c;                       // achieved_t: goal statistics
    else if (c < od + 2 * gd) k = c - gd;              // goal
    else if (c >= o2 && c < o2 + od) k = c - o2;       // obs_t+1
    else if (c >= o2 + od && c < o2 + od + gd) k = c - o2;      // achieved_t+1
    tab[c] = k >= 0 ? make_float2(mean[k], inv_std[k]) : make_float2(0.0f, 0.0f);
  }
  __syncthreads();
  const long long gtid = (long long)blockIdx.x * 256 + t, nth = (long long)gridDim.x * 256;
  auto one = [&](float x, int c) { const float2 p = tab[c]; return p.y == 0.0f ? x : grx_norm_one(x, p.x, p.y, clip); };
  if ((((uintptr_t)rows ^ (uintptr_t)out) & 15) == 0) {
    long long head = (long long)(((16 - ((uintptr_t)rows & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (gtid < head) out[gtid] = one(rows[gtid], (int)(gtid % W));
    const long long n4 = (n - head) >> 2;
    const float4* s4 = (const float4*)(rows + head);
    float4* d4 = (float4*)(out + head);
    const int step = (int)((nth * 4) % W);
    int col = (int)((head + gtid * 4) % W);
    for (long long i = gtid; i < n4; i += nth) {
      float4 v = s4[i];
      int c = col;
      v.x = one(v.x, c); c = c + 1 == W ? 0 : c + 1;
      v.y = one(v.y, c); c = c + 1 == W ? 0 : c + 1;
      v.z = one(v.z, c); c = c + 1 == W ? 0 : c + 1;
      v.w = one(v.w, c);
      d4[i] = v;
      col += step;
      if (col >= W) col -= W;
    }
    for (long long i = head + (n4 << 2) + gtid; i < n; i += nth) out[i] = one(rows[i], (int)(i % W));
  } else {
    const int step = (int)(nth % W);
    int col = (int)(gtid % W);
    for (long long i = gtid; i < n; i += nth) {
      out[i] = one(rows[i], col);
      col += step;
      if (col >= W) col -= W;
    }
  }
}

// out[r] = [norm(obs) | norm(desired)] of the packed env row r = [obs | achieved | desired | reward | success]: one thread per output column, 256 / D rows per workgroup pass
extern "C" __global__ void __launch_bounds__(256)
grx_norm_apply_packed_kernel(const float* __restrict__ mean, const float* __restrict__ inv_std, const float* __restrict__ packed, float* __restrict__ out, long long n, int PW,
                             int od, int gd, float clip) {
  const int t = threadIdx.x, D = od + gd;
  const int lanes = 256 / D, c = t % D, lane = t / D;
  if (lane >= lanes) return;
  const int col = c < od ? c : c + gd;
  const float m = mean[c], s = inv_std[c];
  for (long long r = (long long)blockIdx.x * lanes + lane; r < n; r += (long long)gridDim.x * lanes) out[r * D + c] = grx_norm_one(packed[r * PW + col], m, s, clip);
}

// ---------------------------------------------------------------------------------------------------- host entry points (include/grx_capi.h)
static int grx_norm_check_dims(const char* who, int obs_dim, int goal_dim) {
  if (obs_dim < 1 || goal_dim < 1) return fail(std::string(who) + ": obs_dim and goal_dim must be at least 1");
  if (obs_dim + goal_dim > kNormMaxD) return fail(std::string(who) + ": obs_dim + goal_dim = " + std::to_string(obs_dim + goal_dim) + " exceeds " + std::to_string(kNormMaxD));
  return 0;
}

extern "C" int grx_normstat_geometry(int* rows_per_group, int* max_groups) {
  if (rows_per_group) *rows_per_group = kNormRows;
  if (max_groups) *max_groups = kNormGroups;
  return 0;
}

extern "C" int grx_normstat_layout(int obs_dim, int goal_dim, int64_t* out8) {
  if (!out8) return fail("grx_normstat_layout: null argument");
  if (grx_norm_check_dims("grx_normstat_layout", obs_dim, goal_dim) != 0) return -1;
  const GrxNormLayout L = grx_norm_layout(obs_dim + goal_dim);
  out8[0] = L.sum; out8[1] = L.sumsq; out8[2] = L.count; out8[3] = L.skipped; out8[4] = L.mean; out8[5] = L.inv_std; out8[6] = L.public_bytes; out8[7] = L.total_bytes;
  return 0;
}

static int grx_norm_finish(void* stats, int D, int ngroups, long long batch, const int32_t* valid, double eps, void* stream) {
  const GrxNormLayout L = grx_norm_layout(D);
  char* b = (char*)stats;
  hipLaunchKernelGGL(grx_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (double*)(b + L.sum), (long long*)(b + L.count), (long long*)(b + L.skipped),
                     (float*)(b + L.mean), (float*)(b + L.inv_std), (const double*)(b + L.partial), (const long long*)(b + L.pskip), ngroups, batch, D, (const int*)valid, eps);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int grx_normstat_update(void* stats, const float* rows, int64_t batch, int row_width, int obs_dim, int goal_dim, const int32_t* valid, double eps, void* stream) {
  if (!stats || !rows) return fail("grx_normstat_update: null buffer");
  if (grx_norm_check_dims("grx_normstat_update", obs_dim, goal_dim) != 0) return -1;
  if (batch < 1) return fail("grx_normstat_update: batch " + std::to_string((long long)batch) + " out of range (>= 1)");
  if (row_width < obs_dim + 2 * goal_dim || row_width > kNormTile)
    return fail("grx_normstat_update: row_width " + std::to_string(row_width) + " out of range (obs_dim + 2 goal_dim .. " + std::to_string(kNormTile) + ")");
  if (!(eps > 0.0)) return fail("grx_normstat_update: eps must be positive");
  const int D = obs_dim + goal_dim;
  const GrxNormLayout L = grx_norm_layout(D);
  const long long chunks = ((long long)batch + kNormRows - 1) / kNormRows;
  const int ngroups = (int)(chunks < kNormGroups ? chunks : kNormGroups);
  GrxNormUpdateArgs a;
  a.rows = rows; a.batch = (long long)batch; a.W = row_width; a.od = obs_dim; a.gd = goal_dim; a.valid = (const int*)valid;
  a.partial = (double*)((char*)stats + L.partial); a.pskip = (long long*)((char*)stats + L.pskip);
  hipLaunchKernelGGL(grx_norm_update_kernel, dim3((unsigned)ngroups), dim3(256), 0, (hipStream_t)stream, a);
  HIP_OK(hipGetLastError());
  return grx_norm_finish(stats, D, ngroups, (long long)batch, valid, eps, stream);
}

extern "C" int grx_normstat_refresh(void* stats, int obs_dim, int goal_dim, double eps, void* stream) {
  if (!stats) return fail("grx_normstat_refresh: null buffer");
  if (grx_norm_check_dims("grx_normstat_refresh", obs_dim, goal_dim) != 0) return -1;
  if (!(eps > 0.0)) return fail("grx_normstat_refresh: eps must be positive");
  return grx_norm_finish(stats, obs_dim + goal_dim, 0, 0, nullptr, eps, stream);
}

extern "C" int grx_normstat_apply_batch(const void* stats, const float* rows, int64_t batch, int row_width, int obs_dim, int goal_dim, int act_dim, float clip, float* out,
                                        void* stream) {
  if (!stats || !rows || !out) return fail("grx_normstat_apply_batch: null buffer");
  if (grx_norm_check_dims("grx_normstat_apply_batch", obs_dim, goal_dim) != 0) return -1;
  if (batch < 1) return fail("grx_normstat_apply_batch: batch " + std::to_string((long long)batch) + " out of range (>= 1)");
  if (act_dim < 0 || row_width != 2 * obs_dim + 3 * goal_dim + act_dim + 2 || row_width > kNormMaxWidth)
    return fail("grx_normstat_apply_batch: row_width " + std::to_string(row_width) + " is not 2 obs_dim + 3 goal_dim + act_dim + 2, or exceeds " + std::to_string(kNormMaxWidth));
  if (!(clip > 0.0f)) return fail("grx_normstat_apply_batch: clip must be positive");
  const GrxNormLayout L = grx_norm_layout(obs_dim + goal_dim);
  const char* b = (const char*)stats;
  const long long n = (long long)batch * row_width;
  long long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(grx_norm_apply_batch_kernel, dim3((unsigned)blocks), dim3(256), (size_t)row_width * sizeof(float2), (hipStream_t)stream, (const float*)(b + L.mean),
                     (const float*)(b + L.inv_std), rows, out, n, row_width, obs_dim, goal_dim, act_dim, clip);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int grx_normstat_apply_packed(const void* stats, const float* packed, int64_t n, int packed_width, int obs_dim, int goal_dim, float clip, float* out, void* stream) {
  if (!stats || !packed || !out) return fail("grx_normstat_apply_packed: null buffer");
  if (grx_norm_check_dims("grx_normstat_apply_packed", obs_dim, goal_dim) != 0) return -1;
  if (n < 1) return fail("grx_normstat_apply_packed: n " + std::to_string((long long)n) + " out of range (>= 1)");
  if (packed_width < obs_dim + 2 * goal_dim) return fail("grx_normstat_apply_packed: packed_width " + std::to_string(packed_width) + " is less than obs_dim + 2 goal_dim");
  if (!(clip > 0.0f)) return fail("grx_normstat_apply_packed: clip must be positive");
  const int D = obs_dim + goal_dim, lanes = 256 / D;
  const GrxNormLayout L = grx_norm_layout(D);
  const char* b = (const char*)stats;
  long long blocks = ((long long)n + lanes - 1) / lanes;
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(grx_norm_apply_packed_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)(b + L.mean), (const float*)(b + L.inv_std), packed,
                     out, (long long)n, packed_width, obs_dim, goal_dim, clip);
  HIP_OK(hipGetLastError());
  return 0;
}
