// inr_sample.hip -- weighted epochs: the rows of an epoch drawn with probability proportional to a
// per-row weight.  Two steps, both integer arithmetic after ONE fp64 product per row, so that the results depend neither
// on a summation order nor on a launch shape and inr_mi355x/sampling.py restates them bit for bit:
//
//   inr_row_cdf       ticks q_i = 0 where mask[i] == 0 or !(w_i > 0) (NaN, negative, +-0), else
//                     min(2^32 - 1, floor(fp64(w_i) * scale)); cdf[i] = q_0 + ... + q_i as uint64.
//   inr_sample_epoch  position j holds stratum s = order_m(j) (shuffle_order over [0, m)); with T = cdf[n-1] and
//                     stride = T div m the stratum's threshold is t = s * stride + (u_s mod stride), u_s two MIX words of
//                     s under the draw keys; the row is the smallest i with cdf[i] > t.  Then the gather of epoch_row.
//
// The scan takes three launches -- per-tile sums, one workgroup over the tile sums, per-tile scan plus offset -- and
// reads w twice.  A single-pass scan (chained or decoupled look-back) reads it once, but a tile there WAITS for a flag
// its predecessor sets: it is correct only while the predecessor is resident or scheduled first, which no launch
// promises, and a wait that never ends hangs the device for everyone on it.  Here no workgroup waits on another, there
// is no flag, and every loop has a bound known at launch.  The second read of w (14 MB at the brain shape) comes from
// the Infinity Cache.
#include "inr_epoch_rows.h"

namespace inr {

namespace {

constexpr int CDF_THREADS = 256;
constexpr int CDF_WAVES = CDF_THREADS / 64;
constexpr int CDF_LANE_ROWS = 4;
constexpr int CDF_TILE = CDF_THREADS * CDF_LANE_ROWS;  // 1024 rows per workgroup
using u64 = unsigned long long;

__device__ __forceinline__ unsigned row_ticks(float w, unsigned mask_byte, double scale) {
  if (mask_byte == 0u || !(w > 0.f)) return 0u;
  const double p = (double)w * scale;  // > 0 or +inf: truncation is floor
  return p >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)p;
}

// the four ticks of a lane: rows r .. r + 3 of the tile (rows at or beyond n have none).  VEC: w is 16-byte aligned and
// mask 4-byte aligned
template <bool VEC>
__device__ __forceinline__ void lane_ticks(const float* __restrict__ w, const uint8_t* __restrict__ mask, unsigned r,
                                           unsigned n, double scale, unsigned q[CDF_LANE_ROWS]) {
  if (VEC && r + CDF_LANE_ROWS <= n) {
    const float4 w4 = *reinterpret_cast<const float4*>(w + r);
    const unsigned m = mask != nullptr ? *reinterpret_cast<const unsigned*>(mask + r) : 0x01010101u;
    q[0] = row_ticks(w4.x, m & 0xFFu, scale);
    q[1] = row_ticks(w4.y, (m >> 8) & 0xFFu, scale);
    q[2] = row_ticks(w4.z, (m >> 16) & 0xFFu, scale);
    q[3] = row_ticks(w4.w, m >> 24, scale);
  } else {
#pragma unroll
    for (int j = 0; j < CDF_LANE_ROWS; ++j)
      q[j] = r + j < n ? row_ticks(w[r + j], mask != nullptr ? mask[r + j] : 1u, scale) : 0u;
  }
}

__device__ __forceinline__ u64 wave_inclusive(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// inclusive scan of one value per thread over the block; *total = the block's sum
__device__ __forceinline__ u64 block_inclusive(u64 v, u64* total) {
  __shared__ u64 wave_sum[CDF_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_inclusive(v, lane);
  __syncthreads();  // the previous use of wave_sum is over
  if (lane == 63) wave_sum[wave] = v;
  __syncthreads();
  u64 before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < CDF_WAVES; ++k) {
    if (k < wave) before += wave_sum[k];
    all += wave_sum[k];
  }
  *total = all;
  return v + before;
}

// pass 1: sums[tile] = ticks of the tile
template <bool VEC>
__global__ __launch_bounds__(CDF_THREADS) void row_cdf_sums_kernel(const float* __restrict__ w,
                                                                    const uint8_t* __restrict__ mask, unsigned n,
                                                                    double scale, u64* __restrict__ sums) {
  unsigned q[CDF_LANE_ROWS];
  lane_ticks<VEC>(w, mask, blockIdx.x * (unsigned)CDF_TILE + threadIdx.x * CDF_LANE_ROWS, n, scale, q);
  u64 total;
  block_inclusive((u64)q[0] + q[1] + q[2] + q[3], &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// pass 2: one workgroup turns sums[0 .. tiles) into the ticks in front of each tile, CDF_TILE of them per round
// (ceil(tiles / CDF_TILE) rounds: 2048 at n = 2^31 - 1)
__global__ __launch_bounds__(CDF_THREADS) void row_cdf_offsets_kernel(u64* __restrict__ sums, unsigned tiles) {
  u64 carry = 0;
  for (unsigned base = 0; base < tiles; base += CDF_TILE) {
    const unsigned r = base + threadIdx.x * CDF_LANE_ROWS;
    u64 v[CDF_LANE_ROWS];
#pragma unroll
    for (int j = 0; j < CDF_LANE_ROWS; ++j) v[j] = r + j < tiles ? sums[r + j] : 0;
    u64 total;
    const u64 incl = block_inclusive(v[0] + v[1] + v[2] + v[3], &total);
    u64 run = carry + incl - (v[0] + v[1] + v[2] + v[3]);  // exclusive
#pragma unroll
    for (int j = 0; j < CDF_LANE_ROWS; ++j) {
      if (r + j < tiles) sums[r + j] = run;
      run += v[j];
    }
    carry += total;
  }
}

// pass 3: cdf of the tile = the ticks in front of it + the scan inside it
template <bool VEC>
__global__ __launch_bounds__(CDF_THREADS) void row_cdf_scan_kernel(const float* __restrict__ w,
                                                                    const uint8_t* __restrict__ mask, unsigned n,
                                                                    double scale, const u64* __restrict__ offsets,
                                                                    u64* __restrict__ cdf) {
  const unsigned r = blockIdx.x * (unsigned)CDF_TILE + threadIdx.x * CDF_LANE_ROWS;
  unsigned q[CDF_LANE_ROWS];
  lane_ticks<VEC>(w, mask, r, n, scale, q);
  const u64 mine = (u64)q[0] + q[1] + q[2] + q[3];
  u64 total;
  u64 run = offsets[blockIdx.x] + block_inclusive(mine, &total) - mine;
  u64 c[CDF_LANE_ROWS];
#pragma unroll
  for (int j = 0; j < CDF_LANE_ROWS; ++j) c[j] = run += q[j];
  if (VEC && r + CDF_LANE_ROWS <= n) {  // cdf is 16-byte aligned under VEC: two 16-byte stores
    reinterpret_cast<ulonglong2*>(cdf + r)[0] = make_ulonglong2(c[0], c[1]);
    reinterpret_cast<ulonglong2*>(cdf + r)[1] = make_ulonglong2(c[2], c[3]);
  } else {
#pragma unroll
    for (int j = 0; j < CDF_LANE_ROWS; ++j)
      if (r + j < n) cdf[r + j] = c[j];
  }
}

// One thread per output row.  The search is at most 31 dependent 8-byte loads (n < 2^31); its first levels touch the
// same few words in every lane and stay in the caches, the last ones are one word anywhere in the table.
__global__ __launch_bounds__(256) void sample_epoch_kernel(const ShuffleKeys sk, const DrawKeys dk,
                                                           const u64* __restrict__ cdf, unsigned n, unsigned m,
                                                           unsigned bs, const float* __restrict__ coords,
                                                           const float* __restrict__ gt, const float* __restrict__ dist,
                                                           const uint8_t* __restrict__ mask,
                                                           float* __restrict__ coords_out, float* __restrict__ gt_out,
                                                           float* __restrict__ dist_out, uint8_t* __restrict__ mask_out,
                                                           int* __restrict__ batch_counts,
                                                           long long* __restrict__ order_out) {
  const u64 jj = (u64)blockIdx.x * 256 + threadIdx.x;
  const bool live = jj < m;
  unsigned lo = 0;
  if (live) {
    const u64 T = cdf[n - 1];
    const u64 stride = T / m;
    u64 t = 0;  // stride == 0 (T < m): every position takes the row of threshold 0
    if (stride != 0) {
      const unsigned s = shuffle_order(sk, (unsigned)jj, m);
      const u64 u = ((u64)shuffle_mix(s ^ dk.k[0]) << 32) | shuffle_mix(s ^ dk.k[1]);
      t = (u64)s * stride + u % stride;  // < m * stride <= T
    }
    if (T != 0) {  // the smallest i with cdf[i] > t exists (cdf[n-1] = T > t); T == 0: row 0
      unsigned hi = n - 1;
      for (int it = 0; it < 32 && lo < hi; ++it) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid; else lo = mid + 1;
      }
    }
  }
  epoch_row(jj, m, bs, live, lo, coords, gt, dist, mask, coords_out, gt_out, dist_out, mask_out, batch_counts,
            order_out);
}

}  // namespace

long long row_cdf_scratch_words(long long n) { return (n + CDF_TILE - 1) / CDF_TILE; }

hipError_t launch_row_cdf(const float* w, const uint8_t* mask, long long n, double scale, unsigned long long* cdf,
                          unsigned long long* scratch, hipStream_t st) {
  const unsigned tiles = (unsigned)row_cdf_scratch_words(n);
  const bool vec = ((((uintptr_t)w | (uintptr_t)cdf) & 15u) | ((uintptr_t)mask & 3u)) == 0;
  if (vec)
    hipLaunchKernelGGL(row_cdf_sums_kernel<true>, dim3(tiles), dim3(CDF_THREADS), 0, st, w, mask, (unsigned)n, scale, scratch);
  else
    hipLaunchKernelGGL(row_cdf_sums_kernel<false>, dim3(tiles), dim3(CDF_THREADS), 0, st, w, mask, (unsigned)n, scale, scratch);
  hipLaunchKernelGGL(row_cdf_offsets_kernel, dim3(1), dim3(CDF_THREADS), 0, st, scratch, tiles);
  if (vec)
    hipLaunchKernelGGL(row_cdf_scan_kernel<true>, dim3(tiles), dim3(CDF_THREADS), 0, st, w, mask, (unsigned)n, scale,
                       (const u64*)scratch, cdf);
  else
    hipLaunchKernelGGL(row_cdf_scan_kernel<false>, dim3(tiles), dim3(CDF_THREADS), 0, st, w, mask, (unsigned)n, scale,
                       (const u64*)scratch, cdf);
  return hipGetLastError();
}

hipError_t launch_sample_epoch(const ShuffleKeys& sk, const DrawKeys& dk, const unsigned long long* cdf, long long n,
                               long long m, long long bs, const float* coords, const float* gt, const float* dist,
                               const uint8_t* mask, float* coords_out, float* gt_out, float* dist_out, uint8_t* mask_out,
                               int* batch_counts, long long* order_out, hipStream_t st) {
  const hipError_t e = epoch_counts_begin(batch_counts, m, &bs, st);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((m + 255) / 256);
  hipLaunchKernelGGL(sample_epoch_kernel, dim3(grid), dim3(256), 0, st, sk, dk, cdf, (unsigned)n, (unsigned)m,
                     (unsigned)bs, coords, gt, dist, mask, coords_out, gt_out, dist_out, mask_out, batch_counts,
                     order_out);
  return hipGetLastError();
}

}  // namespace inr
