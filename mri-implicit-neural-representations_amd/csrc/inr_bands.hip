// inr_bands.hip -- radial band statistics of an [n,2] field in one pass (replaces the per-ring masked
// reductions of clustering.py:48-61, 100-135 and gives the validation epoch its per-ring report).  Row i belongs to band b
// iff lo[b] <= dist[i] <= hi[b] in fp32, both ends included; bands may overlap, nest, be empty.  Per band, as doubles:
//   n, energy = sum |gt|^2, sse = sum |pred - gt|^2, max_abs2 = max fl32(fl32(re re) + fl32(im im)) of gt,
//   max_comp / min_comp = extrema of |gt component|, max_err2 = max |pred - gt|^2.
// Sum terms are formed in fp64 from the fp32 inputs and added in fp64, every operation rounded on its own (no FMA: the
// pragma below); inr_mi355x/bands.py::band_stats_numpy is the same text in numpy.
//
// Mapping: a block of 256 lanes takes `tiles_per_block` consecutive tiles of 1024 rows, a lane 4 consecutive rows of a
// tile -- dist is one 16-B load per lane, gt and pred two each, mask one 4-B load: every input byte is read once and the
// rows stay in registers while the bands are walked.  The band bounds are kernel arguments (scalar loads), the band
// loop is wave-uniform, and a band none of the wave's 256 rows falls into costs one ballot.  Reduction order is fixed:
// lane (rows 0..3) -> wave (xor butterfly 32..1) -> the wave's own LDS slots (lane 0 is the only writer, tiles in
// order) -> block (waves 0..3, one thread per slot) -> scratch [block][band][field] -> band_final_kernel (one block per
// band: strided partials, then a binary tree).  No atomics; two calls give the same bits.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

#pragma clang fp contract(off)  // dr * dr + di * di is three roundings, by definition

namespace inr {

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_WAVES = BD_THREADS / 64;
constexpr int BD_LANE_ROWS = 4;
constexpr int BD_MIN_TILES = 4;      // tiles a block takes at least (when the input has that many)
constexpr int BD_MAX_BLOCKS = 2048;  // beyond 8 Mi rows a block takes more tiles instead
constexpr int F_N = 0, F_ENERGY = 1, F_SSE = 2, F_MAX_ABS2 = 3, F_MAX_COMP = 4, F_MIN_COMP = 5, F_MAX_ERR2 = 6;
static_assert(BAND_FIELDS == 7, "field order of inr_abi.h");
static_assert(BAND_TILE_ROWS == BD_THREADS * BD_LANE_ROWS, "tile");

__device__ inline double field_identity(int f) {
  return f <= F_SSE ? 0.0 : (f == F_MIN_COMP ? (double)INFINITY : -(double)INFINITY);
}

__device__ inline double field_combine(int f, double a, double b) {
  if (f <= F_SSE) return a + b;
  return f == F_MIN_COMP ? fmin(a, b) : fmax(a, b);
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline float wave_maxf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline float wave_minf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// VEC: dist, gt and pred are 16-byte aligned and mask 4-byte aligned
template <bool PRED, bool VEC>
__global__ __launch_bounds__(BD_THREADS) void band_partial_kernel(const BandArgs a, const float* __restrict__ dist,
                                                                   const float* __restrict__ gt,
                                                                   const float* __restrict__ pred,
                                                                   const uint8_t* __restrict__ mask, const unsigned n,
                                                                   const unsigned tiles, const unsigned tiles_per_block,
                                                                   double* __restrict__ part) {
  __shared__ double acc[BD_WAVES][BAND_MAX][BAND_FIELDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.n_bands;
  for (int i = lane; i < K * BAND_FIELDS; i += 64) acc[wave][i / BAND_FIELDS][i % BAND_FIELDS] = field_identity(i % BAND_FIELDS);
  __syncthreads();

  const unsigned t0 = blockIdx.x * tiles_per_block;
  const unsigned t1 = t0 + tiles_per_block < tiles ? t0 + tiles_per_block : tiles;
  for (unsigned tile = t0; tile < t1; ++tile) {
    const unsigned r = tile * (unsigned)BAND_TILE_ROWS + threadIdx.x * BD_LANE_ROWS;  // < 2^31 + 1024
    float d[BD_LANE_ROWS], g[2 * BD_LANE_ROWS], p[2 * BD_LANE_ROWS];
    unsigned m = 0x01010101u;  // one mask byte per row
    if (VEC && r + BD_LANE_ROWS <= n) {
      const float4 d4 = *reinterpret_cast<const float4*>(dist + r);
      const float4 g0 = *reinterpret_cast<const float4*>(gt + 2 * (size_t)r);
      const float4 g1 = *reinterpret_cast<const float4*>(gt + 2 * (size_t)r + 4);
      d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
      g[0] = g0.x, g[1] = g0.y, g[2] = g0.z, g[3] = g0.w, g[4] = g1.x, g[5] = g1.y, g[6] = g1.z, g[7] = g1.w;
      if (PRED) {
        const float4 p0 = *reinterpret_cast<const float4*>(pred + 2 * (size_t)r);
        const float4 p1 = *reinterpret_cast<const float4*>(pred + 2 * (size_t)r + 4);
        p[0] = p0.x, p[1] = p0.y, p[2] = p0.z, p[3] = p0.w, p[4] = p1.x, p[5] = p1.y, p[6] = p1.z, p[7] = p1.w;
      }
      if (mask != nullptr) m = *reinterpret_cast<const unsigned*>(mask + r);
    } else {
#pragma unroll
      for (int j = 0; j < BD_LANE_ROWS; ++j) {
        const bool in = r + j < n;  // rows past the end belong to no band (NaN compares false)
        d[j] = in ? dist[r + j] : NAN;
        g[2 * j] = in ? gt[2 * (size_t)(r + j)] : 0.f;
        g[2 * j + 1] = in ? gt[2 * (size_t)(r + j) + 1] : 0.f;
        if (PRED) {
          p[2 * j] = in ? pred[2 * (size_t)(r + j)] : 0.f;
          p[2 * j + 1] = in ? pred[2 * (size_t)(r + j) + 1] : 0.f;
        }
      }
      if (mask != nullptr) {
        m = 0;
#pragma unroll
        for (int j = 0; j < BD_LANE_ROWS; ++j)
          if (r + j < n) m |= (unsigned)mask[r + j] << (8 * j);
      }
    }
    double en[BD_LANE_ROWS], er[BD_LANE_ROWS];
    float a2[BD_LANE_ROWS], cmax[BD_LANE_ROWS], cmin[BD_LANE_ROWS];
#pragma unroll
    for (int j = 0; j < BD_LANE_ROWS; ++j) {
      if (mask != nullptr && (((m >> (8 * j)) & 0xFFu) != 0u) != (a.mask_select != 0)) d[j] = NAN;
      const float re = g[2 * j], im = g[2 * j + 1];
      en[j] = (double)re * (double)re + (double)im * (double)im;
      a2[j] = re * re + im * im;
      cmax[j] = fmaxf(fabsf(re), fabsf(im));
      cmin[j] = fminf(fabsf(re), fabsf(im));
      if (PRED) {
        const double dr = (double)p[2 * j] - (double)re, di = (double)p[2 * j + 1] - (double)im;
        er[j] = dr * dr + di * di;
      } else {
        er[j] = 0.0;
      }
    }
    for (int b = 0; b < K; ++b) {
      const float lo = a.lo[b], hi = a.hi[b];
      bool in[BD_LANE_ROWS];
      bool any = false;
#pragma unroll
      for (int j = 0; j < BD_LANE_ROWS; ++j) {
        in[j] = d[j] >= lo && d[j] <= hi;
        any |= in[j];
      }
      if (__ballot(any) == 0ull) continue;  // wave-uniform
      double cnt = 0.0, e = 0.0, s = 0.0, me = -(double)INFINITY;
      float ma = -INFINITY, mc = -INFINITY, nc = INFINITY;
#pragma unroll
      for (int j = 0; j < BD_LANE_ROWS; ++j) {
        cnt += (double)__popcll(__ballot(in[j]));  // already the wave's count of row j
        if (in[j]) {
          e += en[j];
          ma = fmaxf(ma, a2[j]);
          mc = fmaxf(mc, cmax[j]);
          nc = fminf(nc, cmin[j]);
          if (PRED) {
            s += er[j];
            me = fmax(me, er[j]);
          }
        }
      }
      e = wave_sum(e);
      ma = wave_maxf(ma);
      mc = wave_maxf(mc);
      nc = wave_minf(nc);
      if (PRED) {
        s = wave_sum(s);
        me = wave_max(me);
      }
      if (lane == 0) {
        double* w = acc[wave][b];
        w[F_N] += cnt;
        w[F_ENERGY] += e;
        w[F_MAX_ABS2] = fmax(w[F_MAX_ABS2], (double)ma);
        w[F_MAX_COMP] = fmax(w[F_MAX_COMP], (double)mc);
        w[F_MIN_COMP] = fmin(w[F_MIN_COMP], (double)nc);
        if (PRED) {
          w[F_SSE] += s;
          w[F_MAX_ERR2] = fmax(w[F_MAX_ERR2], me);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * BAND_FIELDS; i += BD_THREADS) {
    const int b = i / BAND_FIELDS, f = i % BAND_FIELDS;
    double v = acc[0][b][f];
#pragma unroll
    for (int w = 1; w < BD_WAVES; ++w) v = field_combine(f, v, acc[w][b][f]);
    part[(size_t)blockIdx.x * K * BAND_FIELDS + i] = v;
  }
}

// one block per band: stats[b][f] from part[G][K][f]
__global__ __launch_bounds__(BD_THREADS) void band_final_kernel(const double* __restrict__ part, const int G,
                                                                 double* __restrict__ stats) {
  __shared__ double red[BAND_FIELDS][BD_THREADS];
  const int K = gridDim.x, b = blockIdx.x, t = threadIdx.x;
  double v[BAND_FIELDS];
#pragma unroll
  for (int f = 0; f < BAND_FIELDS; ++f) v[f] = field_identity(f);
  for (int g = t; g < G; g += BD_THREADS) {
    const double* p = part + ((size_t)g * K + b) * BAND_FIELDS;
#pragma unroll
    for (int f = 0; f < BAND_FIELDS; ++f) v[f] = field_combine(f, v[f], p[f]);
  }
#pragma unroll
  for (int f = 0; f < BAND_FIELDS; ++f) red[f][t] = v[f];
  __syncthreads();
  // seven fields, sums and extrema, per step: block_reduce (inr_reduce.h) would take seven trees and their barriers
  for (int s = BD_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int f = 0; f < BAND_FIELDS; ++f) red[f][t] = field_combine(f, red[f][t], red[f][t + s]);
    }
    __syncthreads();
  }
  if (t < BAND_FIELDS) stats[b * BAND_FIELDS + t] = red[t][0];
}

struct BandGrid {
  unsigned tiles, tiles_per_block, blocks;
};

// a function of n alone, so that scratch is sized without a device query
BandGrid band_grid(long long n) {
  BandGrid g;
  g.tiles = (unsigned)((n + BAND_TILE_ROWS - 1) / BAND_TILE_ROWS);
  const unsigned spread = (g.tiles + BD_MAX_BLOCKS - 1) / BD_MAX_BLOCKS;
  g.tiles_per_block = spread > (unsigned)BD_MIN_TILES ? spread : (unsigned)BD_MIN_TILES;
  g.blocks = (g.tiles + g.tiles_per_block - 1) / g.tiles_per_block;
  return g;
}

}  // namespace

long long band_stats_scratch_doubles(long long n, int n_bands) {
  return (long long)band_grid(n).blocks * n_bands * BAND_FIELDS;
}

hipError_t launch_band_stats(const BandArgs& a, const float* dist, const float* gt, const float* pred,
                             const uint8_t* mask, long long n, double* stats, double* scratch, hipStream_t st) {
  const BandGrid g = band_grid(n);
  const bool vec = ((((uintptr_t)dist | (uintptr_t)gt | (uintptr_t)pred) & 15u) | ((uintptr_t)mask & 3u)) == 0;
#define INR_BAND_LAUNCH(P, V)                                                                                        \
  hipLaunchKernelGGL((band_partial_kernel<P, V>), dim3(g.blocks), dim3(BD_THREADS), 0, st, a, dist, gt, pred, mask, \
                     (unsigned)n, g.tiles, g.tiles_per_block, scratch)
  if (pred != nullptr) {
    if (vec) INR_BAND_LAUNCH(true, true); else INR_BAND_LAUNCH(true, false);
  } else {
    if (vec) INR_BAND_LAUNCH(false, true); else INR_BAND_LAUNCH(false, false);
  }
#undef INR_BAND_LAUNCH
  hipLaunchKernelGGL(band_final_kernel, dim3(a.n_bands), dim3(BD_THREADS), 0, st, scratch, (int)g.blocks, stats);
  return hipGetLastError();
}

}  // namespace inr
