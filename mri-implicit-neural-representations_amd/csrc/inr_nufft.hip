// inr_nufft.hip -- table-based (Kaiser-Bessel) gridding: the operators of inr_nudft / inr_adjoint_nudft approximated in
// O(M J^2 + G log G) instead of O(M H W) (no reference counterpart).  Fixed parameters: oversampling 2
// (Gy = 2 H, Gx = 2 W), J = 6 taps per axis, kb(t) = I0(beta sqrt(1 - (2 t / J)^2)) / I0(beta) on |t| <= J / 2,
// beta = pi sqrt((J / 2)^2 (2 - 1/2)^2 - 0.8) (Beatty et al. 2005).  A sample at index position u sits at
// g = 2 (u - c) + G / 2 on the oversampled grid (c = n / 2, integer division), reduced into [0, G); its taps are the cells
// j0 .. j0 + 5, j0 = ceil(g - 3), wrapped modulo G, with weights kb(g - j).  The FFT between the calls is the caller's
// (torch.fft in inr_mi355x/trajectory.py, which also restates all of this in fp64: nufft_numpy, nufft_adjoint_numpy).
//
//   nufft_taps_kernel     per sample j0y, j0x and the 2 x 6 weights into scratch, once for all coils: offset and I0 in
//                         fp64 (power series, 40 terms: the first neglected one is below 1e-19 of the sum at beta), the
//                         weight stored as fp32.  Scratch is [14][Mp], Mp = M rounded up to 64, every entry written.
//   nufft_prepare_kernel  img [C][H][W][2] times 2 / (a_y[y] a_x[x]), centred in the zero grid [C][Gy][Gx][2]; one
//                         thread per two grid cells (16-byte stores).  The 2 is sqrt(Gy Gx) / sqrt(H W): the caller's FFT
//                         is orthonormal.
//   nufft_finish_kernel   the other way: the centre H x W of grid times 2 / (a_y[y] a_x[x]).
//   nufft_interp_kernel   forward gather, a sample per lane: taps read once, then for every coil the 36 cells in the
//                         order ky, kx.
//   (interp and spread take the grid centred, or -- PLAIN, DESIGN.md 4.31 -- as a plain FFT lays it out)
//   nufft_spread_kernel   the adjoint as a gather, no atomics: a workgroup owns a 16 x 16 tile of grid cells for up to
//                         four coils, a thread one cell.  Samples come sorted into bins of 16 x 16 cells by the cell
//                         that holds floor(g) (trajectory.nufft_bins: bin_start [T + 1], order [M]); the taps of such
//                         a sample lie in floor(g) - 3 .. floor(g) + 3 per axis, so the tile walks the bins that hold a
//                         cell of [lo - 3, hi + 3] modulo G per axis -- at most four per axis, narrow last bin
//                         included -- in ascending bin order and ascending list order, 64 samples at a time through
//                         LDS.  The order of additions per cell is fixed: two calls give the same bits.  A bin may be
//                         of any length.  Entries of bin_start are clamped to [0, M] and an order[] entry outside
//                         [0, M) adds zeros, so malformed bins lose samples but read nothing out of bounds.
// LDS image of a chunk: j0y, j0x [64]; weights [64][6] per axis (a thread reads row s at its own ky: six consecutive
// banks, everything else broadcasts); w * val [4][64] pairs.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

namespace inr {

namespace {

constexpr int NF_J = NUFFT_TAPS;
constexpr int NF_T = NUFFT_TILE;   // cells per tile edge = cells per bin edge
constexpr int NF_THREADS = 256;
constexpr int NF_CHUNK = 64;       // samples staged at a time
constexpr int NF_CG = 4;           // coils per spread workgroup
constexpr int NF_MPAD = 64;
constexpr int NF_I0_TERMS = 40;
constexpr int NF_MAXB = 8;         // bins per axis a tile can reach (4 by the argument above)
constexpr double NF_BETA = 13.85508529027538;  // pi sqrt(9 * 2.25 - 0.8)

static_assert(NF_T * NF_T == NF_THREADS, "a thread per cell");
static_assert(NF_THREADS == 4 * NF_CHUNK, "four staging jobs of one wave each");

__device__ inline double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
#pragma unroll
  for (int k = 1; k <= NF_I0_TERMS; ++k) {
    term *= q * (1.0 / ((double)k * (double)k));
    sum += term;
  }
  return sum;
}

// one axis of one sample: the first tap and the six weights
__device__ inline void axis_taps(double u, int n, int* j0, float* wgt) {
  const double G = 2.0 * (double)n;
  double g = 2.0 * (u - (double)(n / 2)) + (double)n;
  g = g - G * floor(g / G);
  if (g >= G) g -= G;
  if (!(g >= 0.0 && g < G)) g = 0.0;  // a position that is not finite, or too large to reduce: no tap leaves the grid
  const double first = ceil(g - 0.5 * NF_J);
  const double inv_i0 = 1.0 / bessel_i0(NF_BETA);
#pragma unroll
  for (int k = 0; k < NF_J; ++k) {
    const double t = (g - (first + (double)k)) * (2.0 / NF_J);
    const double r = fmax(0.0, 1.0 - t * t);
    wgt[k] = (float)(bessel_i0(NF_BETA * sqrt(r)) * inv_i0);
  }
  *j0 = (int)first;
}

__global__ __launch_bounds__(NF_THREADS) void nufft_taps_kernel(const double* __restrict__ pos, const long long M,
                                                                 const long long Mp, const int H, const int W,
                                                                 float* __restrict__ taps) {
  const long long m = (long long)blockIdx.x * NF_THREADS + threadIdx.x;
  if (m >= Mp) return;
  int jy = 0, jx = 0;
  float wy[NF_J], wx[NF_J];
#pragma unroll
  for (int k = 0; k < NF_J; ++k) wy[k] = wx[k] = 0.f;
  if (m < M) {
    axis_taps(pos[2 * m], H, &jy, wy);
    axis_taps(pos[2 * m + 1], W, &jx, wx);
  }
  int* ti = reinterpret_cast<int*>(taps);
  ti[m] = jy;
  ti[Mp + m] = jx;
#pragma unroll
  for (int k = 0; k < NF_J; ++k) {
    taps[(2 + k) * Mp + m] = wy[k];
    taps[(2 + NF_J + k) * Mp + m] = wx[k];
  }
}

__global__ __launch_bounds__(NF_THREADS) void nufft_prepare_kernel(const float* __restrict__ img,
                                                                    const float* __restrict__ apod_y,
                                                                    const float* __restrict__ apod_x, const int H,
                                                                    const int W, const long long n_pairs,
                                                                    float* __restrict__ grid) {
  const long long i = (long long)blockIdx.x * NF_THREADS + threadIdx.x;  // pair i: cells 2 i, 2 i + 1 of one row
  if (i >= n_pairs) return;
  const long long row = i / W;  // c * Gy + gy: a row holds Gx / 2 = W pairs
  const int gx = 2 * (int)(i - row * W);
  const long long c = row / (2LL * H);
  const int gy = (int)(row - c * 2LL * H);
  const int y = gy - H + H / 2;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (y >= 0 && y < H) {
    const float ay = apod_y[y];
    const float* src = img + 2 * ((size_t)c * H + y) * W;
    const int x0 = gx - W + W / 2;
    if (x0 >= 0 && x0 < W) {
      const float2 v = *reinterpret_cast<const float2*>(src + 2 * (size_t)x0);
      const float d = deapodise(ay, apod_x[x0]);
      o.x = v.x * d;
      o.y = v.y * d;
    }
    if (x0 + 1 >= 0 && x0 + 1 < W) {
      const float2 v = *reinterpret_cast<const float2*>(src + 2 * (size_t)(x0 + 1));
      const float d = deapodise(ay, apod_x[x0 + 1]);
      o.z = v.x * d;
      o.w = v.y * d;
    }
  }
  *reinterpret_cast<float4*>(grid + 4 * (size_t)i) = o;
}

__global__ __launch_bounds__(NF_THREADS) void nufft_finish_kernel(const float* __restrict__ grid,
                                                                   const float* __restrict__ apod_y,
                                                                   const float* __restrict__ apod_x, const int H,
                                                                   const int W, const long long n, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * NF_THREADS + threadIdx.x;  // pixel (c, y, x)
  if (i >= n) return;
  const long long row = i / W;  // c * H + y
  const int x = (int)(i - row * W);
  const long long c = row / H;
  const int y = (int)(row - c * H);
  const size_t src = ((size_t)c * 2 * H + (size_t)(y - H / 2 + H)) * 2 * W + (size_t)(x - W / 2 + W);
  const float2 v = *reinterpret_cast<const float2*>(grid + 2 * src);
  const float d = deapodise(apod_y[y], apod_x[x]);
  *reinterpret_cast<float2*>(out + 2 * (size_t)i) = make_float2(v.x * d, v.y * d);
}

// PLAIN (both kernels below): the grid in the layout of a plain FFT, the centred one rolled by (Gy / 2, Gx / 2)
template <bool PLAIN>
__global__ __launch_bounds__(NF_THREADS) void nufft_interp_kernel(const float* __restrict__ grid,
                                                                   const float* __restrict__ taps, const long long M,
                                                                   const long long Mp, const int C, const int Gy,
                                                                   const int Gx, float* __restrict__ out) {
  const long long m = (long long)blockIdx.x * NF_THREADS + threadIdx.x;
  if (m >= M) return;
  const int* ti = reinterpret_cast<const int*>(taps);
  const int jy = ti[m], jx = ti[Mp + m];
  float wy[NF_J], wx[NF_J];
  size_t rowy[NF_J];
  int colx[NF_J];
#pragma unroll
  for (int k = 0; k < NF_J; ++k) {
    wy[k] = taps[(2 + k) * Mp + m];
    wx[k] = taps[(2 + NF_J + k) * Mp + m];
    int y = jy + k, x = jx + k;  // j0 in [-3, G - 3] and G >= 6: one wrap either way
    y += y < 0 ? Gy : 0;
    y -= y >= Gy ? Gy : 0;
    x += x < 0 ? Gx : 0;
    x -= x >= Gx ? Gx : 0;
    if constexpr (PLAIN) {
      y += y < Gy / 2 ? Gy / 2 : -(Gy / 2);
      x += x < Gx / 2 ? Gx / 2 : -(Gx / 2);
    }
    rowy[k] = (size_t)y * Gx;
    colx[k] = x;
  }
  const size_t plane = (size_t)Gy * Gx;
  for (int c = 0; c < C; ++c) {
    const float* gc = grid + 2 * (size_t)c * plane;
    float ar = 0.f, ai = 0.f;
#pragma unroll
    for (int ky = 0; ky < NF_J; ++ky) {
#pragma unroll
      for (int kx = 0; kx < NF_J; ++kx) {
        const float2 f = *reinterpret_cast<const float2*>(gc + 2 * (rowy[ky] + colx[kx]));
        const float wgt = wy[ky] * wx[kx];
        ar = fmaf(wgt, f.x, ar);
        ai = fmaf(wgt, f.y, ai);
      }
    }
    *reinterpret_cast<float2*>(out + 2 * ((size_t)c * M + m)) = make_float2(ar, ai);
  }
}

// the bins of one axis that hold a cell of [lo - 3, hi + 3] modulo G, ascending and distinct (uniform per workgroup)
__device__ inline int reach_bins(int tile, int G, int* list) {
  const int lo = tile * NF_T - NF_J / 2;
  const int hi = min(tile * NF_T + NF_T - 1, G - 1) + NF_J / 2;
  int n = 0;
  for (int cell = lo; cell <= hi; ++cell) {
    int cm = cell % G;
    cm += cm < 0 ? G : 0;
    const int b = cm / NF_T;
    bool seen = false;
    for (int i = 0; i < n; ++i) seen = seen || list[i] == b;
    if (!seen && n < NF_MAXB) {
      int i = n++;
      for (; i > 0 && list[i - 1] > b; --i) list[i] = list[i - 1];
      list[i] = b;
    }
  }
  return n;
}

template <bool PLAIN>
__global__ __launch_bounds__(NF_THREADS) void nufft_spread_kernel(const float* __restrict__ val,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ taps,
                                                                   const int* __restrict__ bin_start,
                                                                   const int* __restrict__ order, const long long M,
                                                                   const long long Mp, const int C, const int Gy,
                                                                   const int Gx, float* __restrict__ grid) {
  __shared__ int sJy[NF_CHUNK], sJx[NF_CHUNK];
  __shared__ float sWy[NF_CHUNK * NF_J], sWx[NF_CHUNK * NF_J];
  __shared__ float2 sV[NF_CG][NF_CHUNK];
  const int t = threadIdx.x, job = t >> 6, s = t & 63;
  const int nbx = (Gx + NF_T - 1) / NF_T;
  const int tile_x = (int)(blockIdx.x % (unsigned)nbx), tile_y = (int)(blockIdx.x / (unsigned)nbx);
  const int c0 = (int)blockIdx.y * NF_CG, nc = min(NF_CG, C - c0);
  const int gy = tile_y * NF_T + (t >> 4), gx = tile_x * NF_T + (t & 15);
  int by[NF_MAXB], bx[NF_MAXB];
  const int nby_reach = reach_bins(tile_y, Gy, by), nbx_reach = reach_bins(tile_x, Gx, bx);
  const int* ti = reinterpret_cast<const int*>(taps);

  float2 acc[NF_CG];
#pragma unroll
  for (int cc = 0; cc < NF_CG; ++cc) acc[cc] = make_float2(0.f, 0.f);

  for (int iy = 0; iy < nby_reach; ++iy) {
    for (int ix = 0; ix < nbx_reach; ++ix) {
      const long long bin = (long long)by[iy] * nbx + bx[ix];
      const long long lo = min(max((long long)bin_start[bin], 0LL), M);
      const long long hi = min(max((long long)bin_start[bin + 1], lo), M);
      for (long long k0 = lo; k0 < hi; k0 += NF_CHUNK) {
        const int count = (int)min((long long)NF_CHUNK, hi - k0);
        __syncthreads();  // the previous chunk has been read
        if (s < count) {
          const long long mo = order[k0 + s];
          const bool ok = mo >= 0 && mo < M;
          const long long m = ok ? mo : 0;
          if (job == 0) {
            sJy[s] = ti[m];
            sJx[s] = ti[Mp + m];
          } else if (job == 1) {
#pragma unroll
            for (int k = 0; k < NF_J; ++k) sWy[s * NF_J + k] = taps[(2 + k) * Mp + m];
          } else if (job == 2) {
#pragma unroll
            for (int k = 0; k < NF_J; ++k) sWx[s * NF_J + k] = taps[(2 + NF_J + k) * Mp + m];
          } else {
            const float wm = w != nullptr ? w[m] : 1.0f;
#pragma unroll
            for (int cc = 0; cc < NF_CG; ++cc) {
              float2 v = make_float2(0.f, 0.f);
              if (cc < nc && ok) {  // an order[] entry outside [0, M) adds zeros
                v = *reinterpret_cast<const float2*>(val + 2 * ((size_t)(c0 + cc) * M + m));
                if (w != nullptr) {
                  v.x *= wm;
                  v.y *= wm;
                }
              }
              sV[cc][s] = v;
            }
          }
        }
        __syncthreads();
        for (int e = 0; e < count; ++e) {
          int ky = gy - sJy[e], kx = gx - sJx[e];  // the tap of sample e on this cell, modulo G
          ky += ky < 0 ? Gy : 0;
          ky -= ky >= Gy ? Gy : 0;
          kx += kx < 0 ? Gx : 0;
          kx -= kx >= Gx ? Gx : 0;
          if (ky >= 0 && ky < NF_J && kx >= 0 && kx < NF_J) {
            const float wgt = sWy[e * NF_J + ky] * sWx[e * NF_J + kx];
#pragma unroll
            for (int cc = 0; cc < NF_CG; ++cc) {
              const float2 v = sV[cc][e];
              acc[cc].x = fmaf(wgt, v.x, acc[cc].x);
              acc[cc].y = fmaf(wgt, v.y, acc[cc].y);
            }
          }
        }
      }
    }
  }
  if (gy < Gy && gx < Gx) {
    const size_t plane = (size_t)Gy * Gx;
    const int sy = PLAIN ? (gy < Gy / 2 ? gy + Gy / 2 : gy - Gy / 2) : gy;  // only the store address moves
    const int sx = PLAIN ? (gx < Gx / 2 ? gx + Gx / 2 : gx - Gx / 2) : gx;
#pragma unroll
    for (int cc = 0; cc < NF_CG; ++cc)
      if (cc < nc) *reinterpret_cast<float2*>(grid + 2 * ((size_t)(c0 + cc) * plane + (size_t)sy * Gx + sx)) = acc[cc];
  }
}

long long padded_samples(long long M) { return (M + NF_MPAD - 1) / NF_MPAD * NF_MPAD; }

void launch_taps(const double* pos, long long M, int H, int W, float* scratch, hipStream_t st) {
  const long long Mp = padded_samples(M);
  hipLaunchKernelGGL(nufft_taps_kernel, dim3((unsigned)(Mp / NF_THREADS + (Mp % NF_THREADS != 0))), dim3(NF_THREADS), 0,
                     st, pos, M, Mp, H, W, scratch);
}

}  // namespace

long long nufft_scratch_floats(long long M) { return (2 + 2 * NF_J) * padded_samples(M); }

hipError_t launch_nufft_prepare(const float* img, const float* apod_y, const float* apod_x, int C, int H, int W,
                                float* grid, hipStream_t st) {
  const long long n_pairs = (long long)C * 2 * H * W;  // C Gy Gx / 2 <= 32 * 2^32 / 2: below 2^31 blocks of 256
  hipLaunchKernelGGL(nufft_prepare_kernel, dim3((unsigned)((n_pairs + NF_THREADS - 1) / NF_THREADS)), dim3(NF_THREADS), 0,
                     st, img, apod_y, apod_x, H, W, n_pairs, grid);
  return hipGetLastError();
}

hipError_t launch_nufft_finish(const float* grid, const float* apod_y, const float* apod_x, int C, int H, int W,
                               float* out, hipStream_t st) {
  const long long n = (long long)C * H * W;
  hipLaunchKernelGGL(nufft_finish_kernel, dim3((unsigned)((n + NF_THREADS - 1) / NF_THREADS)), dim3(NF_THREADS), 0, st,
                     grid, apod_y, apod_x, H, W, n, out);
  return hipGetLastError();
}

hipError_t launch_nufft_interp(const float* grid, const double* pos, int C, int H, int W, long long M, bool plain,
                               float* out, float* scratch, hipStream_t st) {
  launch_taps(pos, M, H, W, scratch, st);
  hipLaunchKernelGGL(plain ? nufft_interp_kernel<true> : nufft_interp_kernel<false>,
                     dim3((unsigned)((M + NF_THREADS - 1) / NF_THREADS)), dim3(NF_THREADS), 0, st, grid, scratch, M,
                     padded_samples(M), C, 2 * H, 2 * W, out);
  return hipGetLastError();
}

hipError_t launch_nufft_spread(const float* val, const double* pos, const float* w, const int* bin_start,
                               const int* order, int C, int H, int W, long long M, bool plain, float* grid, float* scratch,
                               hipStream_t st) {
  launch_taps(pos, M, H, W, scratch, st);
  const unsigned tiles = (unsigned)nufft_bin_count(H, W);
  hipLaunchKernelGGL(plain ? nufft_spread_kernel<true> : nufft_spread_kernel<false>,
                     dim3(tiles, (unsigned)((C + NF_CG - 1) / NF_CG)), dim3(NF_THREADS), 0, st, val, w, scratch, bin_start,
                     order, M, padded_samples(M), C, 2 * H, 2 * W, grid);
  return hipGetLastError();
}

}  // namespace inr
