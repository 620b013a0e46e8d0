// inr_sense_calib.hip -- SENSE fits on CALIBRATED coil maps (no reference counterpart): the maps come
// once from the fully sampled centre of k-space instead of from a second network, and a step needs the image half of
// the adjoint alone.  Three entries, every line of arithmetic one correctly rounded fp32 operation (contraction is
// switched off for this file, as in inr_sense.hip), no atomics, the same bits on every call;
// inr_mi355x/sense_calib.py (lowres_numpy, maps_numpy, sense_adjoint_numpy) is the same text in numpy, bit for bit.
//
//   lowres :  T[c][j][x]   = sum_{i = 0..b-1} kc[c][j][i] * ex[i][x]          (complex, i ascending, from zero)
//             out[c][y][x] = sum_{j = 0..a-1} ey[j][y] * T[c][j][x]           (complex, j ascending, from zero)
//             a complex product u * v:  p0 = ur*vr; p1 = ui*vi; p2 = ur*vi; p3 = ui*vr;  (p0 - p1, p2 + p3)
//             The kernel holds no sine or cosine: ey / ex are the host's phasor tables (float64, phase reduced first).
//   maps   :  r2 = sum_c (re*re + im*im) in coil order, r = sqrtf(r2) -> rss[p];
//             maps[c][p] = low[c][p] / r (IEEE division) where r > floor * max_p r and r > 0, else (0, 0)
//   adjoint:  dimg[p] = sum_g scale * conj(S_g) * gX_g[q]: the dI half of inr_sense_grad alone, same operations per pixel,
//             same coil order, same place q under the shift; reads no img, writes no dsens -- 16 bytes per pixel and
//             coil instead of 32.
//
// Mapping.  lowres: a workgroup of 256 lanes owns one coil, a tile of LR_COLS = 64 columns and LR_ROWS = 64 rows.  It
// builds T for its columns in LDS (a * 64 complex numbers; the array is sized for a = 64, 32 KB: five workgroups fit the
// CU's 160 KB, which is what bounds the occupancy, and 32 KB is below the 64 KB a workgroup may have), then wave w takes
// rows w, w + 4, ...: lane x reads T[j][x] as one 8-byte LDS access (64 consecutive float2: no bank conflict), ey[j][y]
// is the same address for the whole wave.  Every workgroup of a column tile rebuilds T (b / 64 of its own work): the call runs once per fit.
// maps: one lane per pixel loops over the coils, as sense_grad_kernel does.  The maximum is exact (fmaxf is
// order-independent): the first launch writes rss, and in the second every workgroup reduces the whole rss array through
// inr_reduce.h's block reduction before it divides -- no scratch buffer, no host read; skipped when floor == 0.
// adjoint: sense_grad_kernel's mapping (one wave per block, grid-strided, coil loop unrolled by four, two pixels per
// 16-byte access under sense_pairs' rule).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "inr_aux.h"
#include "inr_reduce.h"
#include "inr_sense_ops.h"
#include "inr_sense_place.h"

#pragma clang fp contract(off)

namespace inr {

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_COLS = 64;
constexpr int LR_ROWS = 64;
constexpr int LR_MAX = 64;  // INR_SENSE_CALIB_MAX: a, b <= 64
constexpr int MP_THREADS = 256;
constexpr int MP_MAX_BLOCKS = 1024;

__device__ __forceinline__ void cmul_add(float ur, float ui, float vr, float vi, float& sr, float& si) {
  const float p0 = ur * vr, p1 = ui * vi, p2 = ur * vi, p3 = ui * vr;
  const float re = p0 - p1, im = p2 + p3;
  sr = sr + re, si = si + im;
}

__global__ __launch_bounds__(LR_THREADS) void sense_lowres_kernel(const float2* __restrict__ kc,
                                                                  const float2* __restrict__ ey,
                                                                  const float2* __restrict__ ex, int a, int b,
                                                                  long long Ho, long long Wo, float2* __restrict__ out) {
  __shared__ float2 T[LR_MAX * LR_COLS];
  const int t = threadIdx.x;
  const int xl = t % LR_COLS;
  const long long x = (long long)blockIdx.x * LR_COLS + xl;
  const int c = blockIdx.y;
  const float2* kcc = kc + (long long)c * a * b;
  // stage 1: T[j][xl], lane xl of wave w takes rows j = w, w + 4, ...
  for (int j = t / LR_COLS; j < a; j += LR_THREADS / LR_COLS) {
    float sr = 0.f, si = 0.f;
    if (x < Wo) {
      for (int i = 0; i < b; ++i) {
        const float2 k = kcc[j * b + i];
        const float2 e = ex[(long long)i * Wo + x];
        cmul_add(k.x, k.y, e.x, e.y, sr, si);
      }
    }
    T[j * LR_COLS + xl] = make_float2(sr, si);
  }
  __syncthreads();
  if (x >= Wo) return;
  // stage 2: rows of this workgroup's band
  const long long y0 = (long long)blockIdx.z * LR_ROWS;
  const long long y1 = y0 + LR_ROWS < Ho ? y0 + LR_ROWS : Ho;
  for (long long y = y0 + t / LR_COLS; y < y1; y += LR_THREADS / LR_COLS) {
    float sr = 0.f, si = 0.f;
    for (int j = 0; j < a; ++j) {
      const float2 e = ey[(long long)j * Ho + y];
      const float2 v = T[j * LR_COLS + xl];
      cmul_add(e.x, e.y, v.x, v.y, sr, si);
    }
    out[((long long)c * Ho + y) * Wo + x] = make_float2(sr, si);
  }
}

__global__ __launch_bounds__(MP_THREADS) void sense_rss_kernel(const float2* __restrict__ low, int C, long long P,
                                                               float* __restrict__ rss) {
  for (long long p = (long long)blockIdx.x * MP_THREADS + threadIdx.x; p < P; p += (long long)gridDim.x * MP_THREADS) {
    float r2 = 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      const float2 v = low[(long long)c * P + p];
      const float s0 = v.x * v.x, s1 = v.y * v.y;
      const float s = s0 + s1;
      r2 = r2 + s;
    }
    rss[p] = sqrtf(r2);
  }
}

__global__ __launch_bounds__(MP_THREADS) void sense_maps_kernel(const float2* __restrict__ low, int C, long long P,
                                                                float floor, const float* __restrict__ rss,
                                                                float2* __restrict__ maps) {
  __shared__ float red[MP_THREADS];
  float thr = 0.f;
  if (floor > 0.f) {  // uniform
    float mx = 0.f;   // rss >= 0; fmaxf drops a NaN
    for (long long p = threadIdx.x; p < P; p += MP_THREADS) mx = fmaxf(mx, rss[p]);
    mx = block_reduce<MP_THREADS>(mx, red, MaxF());
    thr = floor * mx;
  }
  for (long long p = (long long)blockIdx.x * MP_THREADS + threadIdx.x; p < P; p += (long long)gridDim.x * MP_THREADS) {
    const float r = rss[p];
    const bool keep = r > thr && r > 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      float2 o = make_float2(0.f, 0.f);
      if (keep) {
        const float2 v = low[(long long)c * P + p];
        o.x = v.x / r, o.y = v.y / r;
      }
      maps[(long long)c * P + p] = o;
    }
  }
}

// sense_grad_kernel's dI half: adjoint_one of inr_sense_ops.h
template <bool PAIR>
__global__ __launch_bounds__(SN_THREADS) void sense_adjoint_kernel(const float* __restrict__ sens,
                                                                   const float* __restrict__ gx, float* __restrict__ dimg,
                                                                   const SenseDims d, const long long units) {
  using V = typename std::conditional<PAIR, float4, float2>::type;
  constexpr int PX = PAIR ? 2 : 1;
  const V* sens_v = reinterpret_cast<const V*>(sens);
  const V* gx_v = reinterpret_cast<const V*>(gx);
  V* dimg_v = reinterpret_cast<V*>(dimg);
  const long long plane_units = d.plane / PX;
  for (long long u = (long long)blockIdx.x * SN_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * SN_THREADS) {
    const long long q = sense_place(d, u * PX) / PX;
    V acc;
    acc.x = 0.f, acc.y = 0.f;
    if constexpr (PAIR) acc.z = 0.f, acc.w = 0.f;
#pragma unroll 4
    for (int g = 0; g < d.G; ++g) {
      const V sv = sens_v[g * plane_units + u];
      const V gv = gx_v[g * plane_units + q];
      adjoint_one(sv.x, sv.y, gv.x, gv.y, d.scale, acc.x, acc.y);
      if constexpr (PAIR) adjoint_one(sv.z, sv.w, gv.z, gv.w, d.scale, acc.z, acc.w);
    }
    dimg_v[u] = acc;
  }
}

}  // namespace

static_assert(LR_MAX == SENSE_CALIB_MAX, "inr_sense_calib.hip and inr_aux.h disagree");

hipError_t launch_sense_lowres(const float* kc, const float* ey, const float* ex, int C, int a, int b, long long Ho,
                               long long Wo, float* out, hipStream_t st) {
  const dim3 grid((unsigned)((Wo + LR_COLS - 1) / LR_COLS), (unsigned)C, (unsigned)((Ho + LR_ROWS - 1) / LR_ROWS));
  hipLaunchKernelGGL(sense_lowres_kernel, grid, dim3(LR_THREADS), 0, st, reinterpret_cast<const float2*>(kc),
                     reinterpret_cast<const float2*>(ey), reinterpret_cast<const float2*>(ex), a, b, Ho, Wo,
                     reinterpret_cast<float2*>(out));
  return hipGetLastError();
}

hipError_t launch_sense_maps(const float* low, int C, long long P, float floor, float* maps, float* rss, hipStream_t st) {
  const long long nb = (P + MP_THREADS - 1) / MP_THREADS;
  const dim3 grid((unsigned)(nb < MP_MAX_BLOCKS ? nb : MP_MAX_BLOCKS));
  hipLaunchKernelGGL(sense_rss_kernel, grid, dim3(MP_THREADS), 0, st, reinterpret_cast<const float2*>(low), C, P, rss);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sense_maps_kernel, grid, dim3(MP_THREADS), 0, st, reinterpret_cast<const float2*>(low), C, P, floor,
                     rss, reinterpret_cast<float2*>(maps));
  return hipGetLastError();
}

hipError_t launch_sense_adjoint(const float* sens, const float* gx, int G, long long H, long long W, float scale, int shift,
                                float* dimg, hipStream_t st) {
  const SenseDims d = sense_dims(G, H, W, scale, shift);
  const bool pair = sense_pairs(W, (uintptr_t)sens | (uintptr_t)gx | (uintptr_t)dimg);
  const long long units = pair ? d.plane / 2 : d.plane;
  if (pair)
    hipLaunchKernelGGL(sense_adjoint_kernel<true>, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, sens, gx, dimg, d,
                       units);
  else
    hipLaunchKernelGGL(sense_adjoint_kernel<false>, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, sens, gx, dimg, d,
                       units);
  return hipGetLastError();
}

}  // namespace inr
