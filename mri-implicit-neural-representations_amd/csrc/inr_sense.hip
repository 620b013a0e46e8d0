// inr_sense.hip -- the product that joins an image network and a coil-sensitivity network in IMAGE space, and its adjoint
// (no reference counterpart).  img [H*W,2] is one complex image, sens [G,H*W,2] the sensitivities of G
// coils, both straight from inr_forward; x / gx [G,H,W,2] are the coil images and the gradient that came back to them.
// Per pixel p = (y, x) and coil g, every line one correctly rounded fp32 operation, in this order:
//   apply:  re = sr*ir - si*ii;   im = sr*ii + si*ir;   x[g][q] = (scale*re, scale*im)
//   grad :  u = (scale*gr, scale*gi)                               (gr, gi) = gx[g][q]
//           dS[g][p] = (ir*ur + ii*ui, ir*ui - ii*ur)              scale * conj(I) * gX
//           dI[p]   += (sr*ur + si*ui, sr*ui - si*ur)              scale * conj(S_g) * gX_g, g = 0..G-1 in this order
// q = p (shift 0), or q = ((y - H/2) mod H, (x - W/2) mod W) (shift 1): the place torch.fft.ifftshift moves pixel p to, so
// that a plain fft2 of x is the centred transform's ifftshift and no shifted copy is ever made.
// inr_mi355x/sense.py (sense_apply_numpy, sense_grad_numpy) is the same text in numpy, bit for bit.
//
// Rounding: contraction is switched off for this file, as in inr_radial_scale.hip (which says why the __f*_rn intrinsics
// are no way to do it), and the definition is written with plain operators; no fast-math flag.
//
// Mapping: streaming kernels, 8 bytes of img per pixel plus 16 (apply) or 24 (grad) per pixel and coil.  One lane owns its
// pixel(s) for every coil: img is read once, dI lives in two (four) registers and is added to in coil order -- no atomics,
// no LDS, no cross-lane step, the same bits on every call.  The launch is sized from H*W alone: blocks of one wave (no
// block-level cooperation exists, and 64-lane blocks spread a plane of a few hundred thousand pixels evenly over the
// CUs), grid-strided beyond SN_MAX_BLOCKS.  The coil loop is unrolled by four so that four coils' loads are in flight per
// lane before the first is used.
//
// Two pixels per lane per 16-byte access when every pointer is 16-byte aligned and W and W/2 are even: then a pair
// (x, x+1) with x even lands on (x', x'+1) with x' even under the shift as well, and every coil plane starts 16-byte
// aligned.  8-byte accesses otherwise.  Both paths do the same arithmetic per pixel.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "inr_aux.h"
#include "inr_sense_ops.h"
#include "inr_sense_place.h"

#pragma clang fp contract(off)

namespace inr {

namespace {

// apply_one: inr_sense_ops.h
__device__ __forceinline__ void grad_one(float ir, float ii, float sr, float si, float gr, float gi, float scale, float& dsr,
                                         float& dsi, float& dir, float& dii) {
  const float ur = scale * gr, ui = scale * gi;
  const float a = ir * ur, b = ii * ui, c = ir * ui, e = ii * ur;
  dsr = a + b, dsi = c - e;
  const float f = sr * ur, h = si * ui, k = sr * ui, l = si * ur;
  const float tr = f + h, ti = k - l;
  dir = dir + tr, dii = dii + ti;
}

// PAIR: a unit is two neighbouring pixels moved as one float4; otherwise one pixel moved as one float2
template <bool PAIR>
__global__ __launch_bounds__(SN_THREADS) void sense_apply_kernel(const float* __restrict__ img, const float* __restrict__ sens,
                                                                 float* __restrict__ x, const SenseDims d,
                                                                 const long long units) {
  using V = typename std::conditional<PAIR, float4, float2>::type;
  constexpr int PX = PAIR ? 2 : 1;
  const V* img_v = reinterpret_cast<const V*>(img);
  const V* sens_v = reinterpret_cast<const V*>(sens);
  V* x_v = reinterpret_cast<V*>(x);
  const long long plane_units = d.plane / PX;
  for (long long u = (long long)blockIdx.x * SN_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * SN_THREADS) {
    const long long q = sense_place(d, u * PX) / PX;
    const V iv = img_v[u];
#pragma unroll 4
    for (int g = 0; g < d.G; ++g) {
      const V sv = sens_v[g * plane_units + u];
      V o;
      if constexpr (PAIR) {
        apply_one(iv.x, iv.y, sv.x, sv.y, d.scale, o.x, o.y);
        apply_one(iv.z, iv.w, sv.z, sv.w, d.scale, o.z, o.w);
      } else {
        apply_one(iv.x, iv.y, sv.x, sv.y, d.scale, o.x, o.y);
      }
      x_v[g * plane_units + q] = o;
    }
  }
}

template <bool PAIR>
__global__ __launch_bounds__(SN_THREADS) void sense_grad_kernel(const float* __restrict__ img, const float* __restrict__ sens,
                                                                const float* __restrict__ gx, float* __restrict__ dimg,
                                                                float* __restrict__ dsens, const SenseDims d,
                                                                const long long units) {
  using V = typename std::conditional<PAIR, float4, float2>::type;
  constexpr int PX = PAIR ? 2 : 1;
  const V* img_v = reinterpret_cast<const V*>(img);
  const V* sens_v = reinterpret_cast<const V*>(sens);
  const V* gx_v = reinterpret_cast<const V*>(gx);
  V* dimg_v = reinterpret_cast<V*>(dimg);
  V* dsens_v = reinterpret_cast<V*>(dsens);
  const long long plane_units = d.plane / PX;
  for (long long u = (long long)blockIdx.x * SN_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * SN_THREADS) {
    const long long q = sense_place(d, u * PX) / PX;
    const V iv = img_v[u];
    V acc;
    acc.x = 0.f, acc.y = 0.f;
    if constexpr (PAIR) acc.z = 0.f, acc.w = 0.f;
#pragma unroll 4
    for (int g = 0; g < d.G; ++g) {
      const V sv = sens_v[g * plane_units + u];
      const V gv = gx_v[g * plane_units + q];
      V o;
      if constexpr (PAIR) {
        grad_one(iv.x, iv.y, sv.x, sv.y, gv.x, gv.y, d.scale, o.x, o.y, acc.x, acc.y);
        grad_one(iv.z, iv.w, sv.z, sv.w, gv.z, gv.w, d.scale, o.z, o.w, acc.z, acc.w);
      } else {
        grad_one(iv.x, iv.y, sv.x, sv.y, gv.x, gv.y, d.scale, o.x, o.y, acc.x, acc.y);
      }
      dsens_v[g * plane_units + u] = o;
    }
    dimg_v[u] = acc;
  }
}

}  // namespace

hipError_t launch_sense_apply(const float* img, const float* sens, int G, long long H, long long W, float scale, int shift,
                              float* x, hipStream_t st) {
  const SenseDims d = sense_dims(G, H, W, scale, shift);
  const bool pair = sense_pairs(W, (uintptr_t)img | (uintptr_t)sens | (uintptr_t)x);
  const long long units = pair ? d.plane / 2 : d.plane;
  if (pair)
    hipLaunchKernelGGL(sense_apply_kernel<true>, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, img, sens, x, d, units);
  else
    hipLaunchKernelGGL(sense_apply_kernel<false>, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, img, sens, x, d, units);
  return hipGetLastError();
}

hipError_t launch_sense_grad(const float* img, const float* sens, const float* gx, int G, long long H, long long W,
                             float scale, int shift, float* dimg, float* dsens, hipStream_t st) {
  const SenseDims d = sense_dims(G, H, W, scale, shift);
  const bool pair = sense_pairs(W, (uintptr_t)img | (uintptr_t)sens | (uintptr_t)gx | (uintptr_t)dimg | (uintptr_t)dsens);
  const long long units = pair ? d.plane / 2 : d.plane;
  if (pair)
    hipLaunchKernelGGL(sense_grad_kernel<true>, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, img, sens, gx, dimg,
                       dsens, d, units);
  else
    hipLaunchKernelGGL(sense_grad_kernel<false>, dim3(sense_blocks(units)), dim3(SN_THREADS), 0, st, img, sens, gx, dimg,
                       dsens, d, units);
  return hipGetLastError();
}

}  // namespace inr
