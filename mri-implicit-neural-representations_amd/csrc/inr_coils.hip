// inr_coils.hip -- software coil compression (no reference counterpart): the coil Gram matrix of a
// coil-major complex scan x [C, N, 2] in one pass, and the streaming product y = A x of an [M, K] complex matrix with
// the K coil rows.  inr_mi355x/coils.py::coil_gram_numpy / coil_apply_numpy are the same text in numpy.
//
// Gram: G[i][j] = sum_p x_i[p] conj(x_j[p]).  The product of two fp32 values is exact in fp64, so
//   re = ar br + ai bi,  im = ai br - ar bi   (each one rounding: an exact product and an fma)
// and everything else is the order of fp64 additions.  That order is fixed:
//   a workgroup of 256 lanes takes `tiles_per_block` consecutive tiles of COIL_TILE_PIXELS pixels of all C coils through
//   LDS (16-byte loads when the coil rows are 16-byte aligned, i.e. N even and an aligned base; 8-byte loads otherwise);
//   a lane owns one pair (i >= j) of the P = C (C + 1) / 2 and, while P <= 128, one of S = 256 / P interleaved pixel
//   slices of the tile (pixels s, s + S, ...), with P > 256 up to three pairs; it adds its terms in pixel order, tiles in
//   order -> the block adds the S slices of a pair in order -> scratch [block][pair][2] -> coil_gram_final_kernel, one
//   block per pair: strided partials, then a binary tree; it writes G[i][j] and the conjugate G[j][i] (diagonal: +0 i).
// No atomics; two calls give the same bits, on any device.  An LDS coil row is padded by one pixel, so the rows a wave
// reads at one pixel sit 2 banks apart (ds_read_b64: conflict-free for up to 32 coils).
//
// Apply: a lane holds 2 pixels (16-byte path) or 1 (8-byte path) of all K coils in registers, the matrix sits in LDS
// and is read wave-uniformly (broadcast); y_m = sum over k = 0..K-1 in order, fp32, re += ar xr - ai xi and
// im += ar xi + ai xr; every input byte is read once, every output byte written once.
#include <hip/hip_runtime.h>
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_ROW = COIL_TILE_PIXELS + 1;  // float2 per LDS coil row
constexpr int CG_MAX_PAIRS = COIL_MAX * (COIL_MAX + 1) / 2;
constexpr int CG_LANE_PAIRS = (CG_MAX_PAIRS + CG_THREADS - 1) / CG_THREADS;  // 3
constexpr int CG_MIN_TILES = 2;      // tiles a block takes at least (when the input has that many)
constexpr int CG_MAX_BLOCKS = 2048;  // beyond that a block takes more tiles instead
static_assert(COIL_TILE_PIXELS % 2 == 0, "a 16-byte load is two pixels of a tile");
static_assert(COIL_MAX * CG_ROW * 8 <= 64 * 1024 && CG_THREADS * 16 <= COIL_MAX * CG_ROW * 8, "LDS");

// pair q = i (i + 1) / 2 + j, i >= j
__device__ inline void pair_of(int q, int& i, int& j) {
  int r = (int)((sqrtf(8.f * (float)q + 1.f) - 1.f) * 0.5f);
  while (r * (r + 1) / 2 > q) --r;
  while ((r + 1) * (r + 2) / 2 <= q) ++r;
  i = r;
  j = q - r * (r + 1) / 2;
}

// VEC: data is 16-byte aligned and N is even (every coil row starts 16-byte aligned, every tile at an even pixel)
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void coil_gram_partial_kernel(const float* __restrict__ x, const int C,
                                                                        const unsigned N, const unsigned tiles,
                                                                        const unsigned tiles_per_block,
                                                                        double* __restrict__ part) {
  extern __shared__ double cg_lds[];  // the tile, then (aliased) the slice partials
  float2* tile = reinterpret_cast<float2*>(cg_lds);
  const int t = threadIdx.x;
  const int P = C * (C + 1) / 2;
  const int S = P <= CG_THREADS ? CG_THREADS / P : 1;
  const int Pm = P < CG_THREADS ? P : CG_THREADS;
  const int s = t / Pm, q0 = t % Pm;
  const bool active = s < S;
  int ci[CG_LANE_PAIRS], cj[CG_LANE_PAIRS];
  double re[CG_LANE_PAIRS], im[CG_LANE_PAIRS];
#pragma unroll
  for (int k = 0; k < CG_LANE_PAIRS; ++k) {
    const int q = q0 + k * CG_THREADS;
    ci[k] = cj[k] = -1;
    if (active && q < P) pair_of(q, ci[k], cj[k]);
    re[k] = im[k] = 0.0;
  }

  const unsigned t0 = blockIdx.x * tiles_per_block;
  const unsigned t1 = t0 + tiles_per_block < tiles ? t0 + tiles_per_block : tiles;
  for (unsigned tl = t0; tl < t1; ++tl) {
    const unsigned p0 = tl * (unsigned)COIL_TILE_PIXELS;  // < 2^31
    if (VEC) {
      constexpr int HALF = COIL_TILE_PIXELS / 2;
      for (int e = t; e < C * HALF; e += CG_THREADS) {
        const int c = e / HALF, pp = 2 * (e % HALF);
        const unsigned p = p0 + pp;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);  // pixels past the end add +0
        if (p < N) v = *reinterpret_cast<const float4*>(x + 2 * ((size_t)c * N + p));  // N even: p + 1 < N too
        tile[c * CG_ROW + pp] = make_float2(v.x, v.y);
        tile[c * CG_ROW + pp + 1] = make_float2(v.z, v.w);
      }
    } else {
      for (int e = t; e < C * COIL_TILE_PIXELS; e += CG_THREADS) {
        const int c = e / COIL_TILE_PIXELS, pp = e % COIL_TILE_PIXELS;
        const unsigned p = p0 + pp;
        float2 v = make_float2(0.f, 0.f);
        if (p < N) v = *reinterpret_cast<const float2*>(x + 2 * ((size_t)c * N + p));
        tile[c * CG_ROW + pp] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CG_LANE_PAIRS; ++k) {
      if (ci[k] < 0) continue;
      const float2* ra = tile + ci[k] * CG_ROW;
      const float2* rb = tile + cj[k] * CG_ROW;
      double r = re[k], m = im[k];
      for (int p = s; p < COIL_TILE_PIXELS; p += S) {
        const float2 a = ra[p], b = rb[p];
        const double ar = (double)a.x, ai = (double)a.y, br = (double)b.x, bi = (double)b.y;
        r += fma(ai, bi, ar * br);
        m += fma(ai, br, -(ar * bi));
      }
      re[k] = r, im[k] = m;
    }
    __syncthreads();
  }

  // slices of a pair, in order (S > 1 only with one pair per lane)
  double* red = cg_lds;
  if (S > 1) {
    red[2 * t] = re[0];
    red[2 * t + 1] = im[0];
    __syncthreads();
    if (s == 0) {
      double r = red[2 * q0], m = red[2 * q0 + 1];
      for (int u = 1; u < S; ++u) {
        r += red[2 * (u * Pm + q0)];
        m += red[2 * (u * Pm + q0) + 1];
      }
      re[0] = r, im[0] = m;
    }
  }
  if (s == 0) {
#pragma unroll
    for (int k = 0; k < CG_LANE_PAIRS; ++k) {
      const int q = q0 + k * CG_THREADS;
      if (q < P) {
        double* w = part + 2 * ((size_t)blockIdx.x * P + q);
        w[0] = re[k];
        w[1] = im[k];
      }
    }
  }
}

struct Cplx {
  double re, im;
};
__device__ inline Cplx operator+(Cplx a, Cplx b) { return {a.re + b.re, a.im + b.im}; }

// one block per pair: G[i][j] and its mirror from part[blocks][P][2]
__global__ __launch_bounds__(CG_THREADS) void coil_gram_final_kernel(const double* __restrict__ part, const int blocks,
                                                                      const int C, double* __restrict__ gram) {
  __shared__ Cplx red[CG_THREADS];
  const int P = gridDim.x, q = blockIdx.x, t = threadIdx.x;
  Cplx v = {0.0, 0.0};
  for (int g = t; g < blocks; g += CG_THREADS) {
    const double* p = part + 2 * ((size_t)g * P + q);
    v.re += p[0];
    v.im += p[1];
  }
  v = block_reduce_once<CG_THREADS>(v, red, Sum());
  if (t == 0) {
    int i, j;
    pair_of(q, i, j);
    const double gr = v.re, gi = i == j ? 0.0 : v.im;
    gram[2 * (i * C + j)] = gr;
    gram[2 * (i * C + j) + 1] = gi;
    if (i != j) {
      gram[2 * (j * C + i)] = gr;
      gram[2 * (j * C + i) + 1] = -gi;
    }
  }
}

struct CoilGrid {
  unsigned tiles, tiles_per_block, blocks;
};

// a function of N alone, so that scratch is sized without a device query
CoilGrid coil_grid(long long N) {
  CoilGrid g;
  g.tiles = (unsigned)((N + COIL_TILE_PIXELS - 1) / COIL_TILE_PIXELS);
  const unsigned spread = (g.tiles + CG_MAX_BLOCKS - 1) / CG_MAX_BLOCKS;
  g.tiles_per_block = spread > (unsigned)CG_MIN_TILES ? spread : (unsigned)CG_MIN_TILES;
  g.blocks = (g.tiles + g.tiles_per_block - 1) / g.tiles_per_block;
  return g;
}

// PIX pixels per lane: 2 with 16-byte loads and stores (N even, aligned bases), else 1.  KR = K rounded up to a multiple
// of 8: the lane's coil registers; the up to 7 rows past K read row K - 1 again (a valid address, a cache hit, never
// used), which keeps every register index static.
template <int PIX, int KR>
__global__ __launch_bounds__(CG_THREADS) void coil_apply_kernel(const float* __restrict__ in,
                                                                 const float* __restrict__ A, const int M, const int K,
                                                                 const unsigned N, float* __restrict__ out) {
  __shared__ float2 sA[COIL_MAX * COIL_MAX];
  for (int e = threadIdx.x; e < M * K; e += CG_THREADS) sA[e] = make_float2(A[2 * e], A[2 * e + 1]);
  __syncthreads();
  const size_t lane0 = ((size_t)blockIdx.x * CG_THREADS + threadIdx.x) * PIX;  // first pixel of this lane
  if (lane0 >= N) return;  // PIX == 2: N is even, so pixel lane0 + 1 exists
  float xr[KR][PIX], xi[KR][PIX];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const float* src = in + 2 * ((size_t)(k < K ? k : K - 1) * N + lane0);
    if (PIX == 2) {
      const float4 v = *reinterpret_cast<const float4*>(src);
      xr[k][0] = v.x, xi[k][0] = v.y, xr[k][PIX - 1] = v.z, xi[k][PIX - 1] = v.w;
    } else {
      const float2 v = *reinterpret_cast<const float2*>(src);
      xr[k][0] = v.x, xi[k][0] = v.y;
    }
  }
  for (int m = 0; m < M; ++m) {
    float yr[PIX], yi[PIX];
#pragma unroll
    for (int u = 0; u < PIX; ++u) yr[u] = yi[u] = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (k < K) {  // wave-uniform
        const float2 a = sA[m * K + k];
#pragma unroll
        for (int u = 0; u < PIX; ++u) {
          yr[u] += a.x * xr[k][u] - a.y * xi[k][u];
          yi[u] += a.x * xi[k][u] + a.y * xr[k][u];
        }
      }
    }
    float* dst = out + 2 * ((size_t)m * N + lane0);
    if (PIX == 2)
      *reinterpret_cast<float4*>(dst) = make_float4(yr[0], yi[0], yr[PIX - 1], yi[PIX - 1]);
    else
      *reinterpret_cast<float2*>(dst) = make_float2(yr[0], yi[0]);
  }
}

template <int PIX>
void coil_apply_launch(const float* in, const float* A, int M, int K, long long N, float* out, hipStream_t st) {
  const long long lanes = N / PIX;
  const dim3 grid((unsigned)((lanes + CG_THREADS - 1) / CG_THREADS)), block(CG_THREADS);
  if (K <= 8)
    hipLaunchKernelGGL((coil_apply_kernel<PIX, 8>), grid, block, 0, st, in, A, M, K, (unsigned)N, out);
  else if (K <= 16)
    hipLaunchKernelGGL((coil_apply_kernel<PIX, 16>), grid, block, 0, st, in, A, M, K, (unsigned)N, out);
  else if (K <= 24)
    hipLaunchKernelGGL((coil_apply_kernel<PIX, 24>), grid, block, 0, st, in, A, M, K, (unsigned)N, out);
  else
    hipLaunchKernelGGL((coil_apply_kernel<PIX, 32>), grid, block, 0, st, in, A, M, K, (unsigned)N, out);
}

}  // namespace

long long coil_gram_scratch_doubles(int C, long long N) {
  return (long long)coil_grid(N).blocks * (C * (C + 1) / 2) * 2;
}

hipError_t launch_coil_gram(const float* data, int C, long long N, double* gram, double* scratch, hipStream_t st) {
  const CoilGrid g = coil_grid(N);
  const int P = C * (C + 1) / 2;
  const size_t tile_bytes = (size_t)C * CG_ROW * sizeof(float2), red_bytes = (size_t)CG_THREADS * 2 * sizeof(double);
  const size_t lds = tile_bytes > red_bytes ? tile_bytes : red_bytes;
  const bool vec = ((uintptr_t)data & 15u) == 0 && N % 2 == 0;
  if (vec)
    hipLaunchKernelGGL(coil_gram_partial_kernel<true>, dim3(g.blocks), dim3(CG_THREADS), lds, st, data, C, (unsigned)N,
                       g.tiles, g.tiles_per_block, scratch);
  else
    hipLaunchKernelGGL(coil_gram_partial_kernel<false>, dim3(g.blocks), dim3(CG_THREADS), lds, st, data, C, (unsigned)N,
                       g.tiles, g.tiles_per_block, scratch);
  hipLaunchKernelGGL(coil_gram_final_kernel, dim3(P), dim3(CG_THREADS), 0, st, scratch, (int)g.blocks, C, gram);
  return hipGetLastError();
}

hipError_t launch_coil_apply(const float* in, const float* A, int M, int K, long long N, float* out, hipStream_t st) {
  const bool vec = ((((uintptr_t)in | (uintptr_t)out) & 15u) == 0) && N % 2 == 0;
  if (vec)
    coil_apply_launch<2>(in, A, M, K, N, out, st);
  else
    coil_apply_launch<1>(in, A, M, K, N, out, st);
  return hipGetLastError();
}

}  // namespace inr
