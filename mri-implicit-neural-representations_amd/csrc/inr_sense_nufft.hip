// inr_sense_nufft.hip -- off-grid SENSE fits on calibrated maps (no reference counterpart): the coil
// product fused with the gridding operators' first and last pass, on a grid laid out as a plain FFT reads and writes
// it, so that a step runs  prepare -> torch.fft.fft2 -> inr_nufft_interp_plain  and
// inr_nufft_spread_plain -> torch.fft.ifft2 -> finish  with no shifted copy and no coil images in between.
//
// The oversampled grid is Gy x Gx = 2H x 2W, even on both axes: fftshift and ifftshift are the same roll by (H, W).
// The centred grid of inr_nufft.hip holds pixel (y, x) at (y - H/2 + H, x - W/2 + W); the plain one holds it at
//   py = (y - H/2) mod 2H,  px = (x - W/2) mod 2W          (integer H/2, W/2)
// so rows [0, H - H/2) are y = H/2 .. H-1, rows [2H - H/2, 2H) are y = 0 .. H/2-1, the rest is padding; columns alike.
//
//   prepare:  x = scale * S_g * I       apply_one's operations in its order (inr_sense_ops.h)
//             grid[g][py][px] = (x.re * d, x.im * d),  d = deapodise(a_y[y], a_x[x])     one rounded product each
//             padding cells are written as zeros: every cell of the grid is written, the caller never clears it
//   finish :  (gr, gi) = grid[g][py][px];  v = (gr * d, gi * d);  adjoint_one(S_g, v, scale) summed into dI in coil
//             order from zero, in registers; dimg[p] = dI, or dimg[p] + dI (one fp32 addition) with `accumulate`
// which is inr_sense_apply(shift 0) + inr_nufft_prepare and inr_nufft_finish + inr_sense_adjoint(shift 0) bit for bit;
// inr_mi355x/sense_nufft.py restates both in fp32 numpy.  No atomics, no LDS, no cross-lane step: same bits every call.
//
// Mapping: streaming kernels.  prepare reads 8 bytes of img and 8 G of maps per pixel and writes 32 G per pixel (the
// grid has four cells per pixel); finish reads 16 G per pixel and writes 8.  One lane owns one grid cell (prepare) or one
// pixel (finish) of every coil, img and d are loaded once, the coil loop is unrolled by four so that four coils' loads
// are in flight before the first is used; blocks of one wave, grid-strided, as in inr_sense.hip.  Two neighbouring cells
// per lane and 16-byte access under sense_pairs' rule (every pointer 16-byte aligned, W and W/2 even): then px is even
// exactly when x is, no pair straddles an edge of the padding, and every coil plane starts 16-byte aligned.  8-byte
// accesses otherwise; both paths do the same arithmetic.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "inr_aux.h"
#include "inr_sense_ops.h"
#include "inr_sense_place.h"

#pragma clang fp contract(off)

namespace inr {

namespace {

struct SenseNufftDims {
  int H, W, G;
  int hh, hw;  // H / 2, W / 2
  float scale;
};

// u = row * per_row + col, per_row > 0; 32-bit division where u fits (uniform per launch)
__device__ __forceinline__ void split_unit(long long u, long long per_row, bool narrow, long long& row, int& col) {
  if (narrow) {
    const unsigned uu = (unsigned)u, pr = (unsigned)per_row;
    const unsigned r = uu / pr;
    row = r, col = (int)(uu - r * pr);
  } else {
    row = u / per_row, col = (int)(u - row * per_row);
  }
}

// the pixel index along one axis of n points that plain cell j of 2 n holds, or -1 for padding
__device__ __forceinline__ int pixel_of_cell(int j, int n, int half) {
  if (j < n - half) return j + half;
  if (j >= 2 * n - half) return j - 2 * n + half;
  return -1;
}

// PAIR: a unit is two neighbouring cells of a row moved as one float4; otherwise one cell moved as one float2
template <bool PAIR>
__global__ __launch_bounds__(SN_THREADS) void sense_nufft_prepare_kernel(const float* __restrict__ img,
                                                                         const float* __restrict__ maps,
                                                                         const float* __restrict__ apod_y,
                                                                         const float* __restrict__ apod_x,
                                                                         const SenseNufftDims d, const long long units,
                                                                         float* __restrict__ grid) {
  using V = typename std::conditional<PAIR, float4, float2>::type;
  constexpr int PX = PAIR ? 2 : 1;
  const V* img_v = reinterpret_cast<const V*>(img);
  const V* maps_v = reinterpret_cast<const V*>(maps);
  V* grid_v = reinterpret_cast<V*>(grid);
  const long long per_row = 2LL * d.W / PX;              // units per grid row
  const long long plane_units = (long long)d.H * d.W / PX;  // units per coil plane of maps
  const long long grid_units = 4 * plane_units;          // ... and of the grid: units == grid_units
  const bool narrow = units <= 0xffffffffLL;
  for (long long u = (long long)blockIdx.x * SN_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * SN_THREADS) {
    long long py;
    int cu;
    split_unit(u, per_row, narrow, py, cu);
    const int y = pixel_of_cell((int)py, d.H, d.hh);
    const int x = pixel_of_cell(cu * PX, d.W, d.hw);  // PAIR: x and x + 1 are pixels together or padding together
    if (y < 0 || x < 0) {
      V z;
      z.x = 0.f, z.y = 0.f;
      if constexpr (PAIR) z.z = 0.f, z.w = 0.f;
      for (int g = 0; g < d.G; ++g) grid_v[g * grid_units + u] = z;
      continue;
    }
    const long long p = ((long long)y * d.W + x) / PX;
    const V iv = img_v[p];
    const float ay = apod_y[y];
    const float d0 = deapodise(ay, apod_x[x]);
    float d1 = 0.f;
    if constexpr (PAIR) d1 = deapodise(ay, apod_x[x + 1]);
#pragma unroll 4
    for (int g = 0; g < d.G; ++g) {
      const V sv = maps_v[g * plane_units + p];
      V o;
      float xr, xi;
      apply_one(iv.x, iv.y, sv.x, sv.y, d.scale, xr, xi);
      o.x = xr * d0, o.y = xi * d0;
      if constexpr (PAIR) {
        apply_one(iv.z, iv.w, sv.z, sv.w, d.scale, xr, xi);
        o.z = xr * d1, o.w = xi * d1;
      }
      grid_v[g * grid_units + u] = o;
    }
  }
}

// PAIR: a unit is two neighbouring pixels of a row; otherwise one
template <bool PAIR, bool ACCUMULATE>
__global__ __launch_bounds__(SN_THREADS) void sense_nufft_finish_kernel(const float* __restrict__ grid,
                                                                        const float* __restrict__ maps,
                                                                        const float* __restrict__ apod_y,
                                                                        const float* __restrict__ apod_x,
                                                                        const SenseNufftDims d, const long long units,
                                                                        float* __restrict__ dimg) {
  using V = typename std::conditional<PAIR, float4, float2>::type;
  constexpr int PX = PAIR ? 2 : 1;
  const V* grid_v = reinterpret_cast<const V*>(grid);
  const V* maps_v = reinterpret_cast<const V*>(maps);
  V* dimg_v = reinterpret_cast<V*>(dimg);
  const long long per_row = (long long)d.W / PX;  // units per image row (PAIR: W is even)
  const long long plane_units = units;            // H * W / PX
  const long long grid_units = 4 * plane_units;
  const bool narrow = units <= 0xffffffffLL;
  for (long long u = (long long)blockIdx.x * SN_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * SN_THREADS) {
    long long y;
    int cu;
    split_unit(u, per_row, narrow, y, cu);
    const int x = cu * PX;
    const long long py = y >= d.hh ? y - d.hh : y - d.hh + 2LL * d.H;
    const long long px = x >= d.hw ? x - d.hw : x - d.hw + 2LL * d.W;  // PAIR: even, and x + 1 lands on px + 1
    const long long q = (py * 2 * d.W + px) / PX;
    const float ay = apod_y[y];
    const float d0 = deapodise(ay, apod_x[x]);
    float d1 = 0.f;
    if constexpr (PAIR) d1 = deapodise(ay, apod_x[x + 1]);
    V acc;
    acc.x = 0.f, acc.y = 0.f;
    if constexpr (PAIR) acc.z = 0.f, acc.w = 0.f;
#pragma unroll 4
    for (int g = 0; g < d.G; ++g) {
      const V sv = maps_v[g * plane_units + u];
      const V gv = grid_v[g * grid_units + q];
      const float vr = gv.x * d0, vi = gv.y * d0;
      adjoint_one(sv.x, sv.y, vr, vi, d.scale, acc.x, acc.y);
      if constexpr (PAIR) {
        const float wr = gv.z * d1, wi = gv.w * d1;
        adjoint_one(sv.z, sv.w, wr, wi, d.scale, acc.z, acc.w);
      }
    }
    if constexpr (ACCUMULATE) {
      const V old = dimg_v[u];
      acc.x = old.x + acc.x, acc.y = old.y + acc.y;
      if constexpr (PAIR) acc.z = old.z + acc.z, acc.w = old.w + acc.w;
    }
    dimg_v[u] = acc;
  }
}

SenseNufftDims sense_nufft_dims(int G, int H, int W, float scale) {
  SenseNufftDims d;
  d.H = H, d.W = W, d.G = G;
  d.hh = H / 2, d.hw = W / 2;
  d.scale = scale;
  return d;
}

}  // namespace

hipError_t launch_sense_nufft_prepare(const float* img, const float* maps, const float* apod_y, const float* apod_x, int G,
                                      int H, int W, float scale, float* grid, hipStream_t st) {
  const SenseNufftDims d = sense_nufft_dims(G, H, W, scale);
  const bool pair = sense_pairs(W, (uintptr_t)img | (uintptr_t)maps | (uintptr_t)grid);
  const long long cells = 4LL * H * W;
  const long long units = pair ? cells / 2 : cells;
  hipLaunchKernelGGL(pair ? sense_nufft_prepare_kernel<true> : sense_nufft_prepare_kernel<false>, dim3(sense_blocks(units)),
                     dim3(SN_THREADS), 0, st, img, maps, apod_y, apod_x, d, units, grid);
  return hipGetLastError();
}

hipError_t launch_sense_nufft_finish(const float* grid, const float* maps, const float* apod_y, const float* apod_x, int G,
                                     int H, int W, float scale, float* dimg, bool accumulate, hipStream_t st) {
  const SenseNufftDims d = sense_nufft_dims(G, H, W, scale);
  const bool pair = sense_pairs(W, (uintptr_t)grid | (uintptr_t)maps | (uintptr_t)dimg);
  const long long plane = (long long)H * W;
  const long long units = pair ? plane / 2 : plane;
  auto kernel = pair ? (accumulate ? sense_nufft_finish_kernel<true, true> : sense_nufft_finish_kernel<true, false>)
                     : (accumulate ? sense_nufft_finish_kernel<false, true> : sense_nufft_finish_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, grid, maps, apod_y, apod_x, d, units, dimg);
  return hipGetLastError();
}

}  // namespace inr
