// inr_sense_ops.h -- the per-pixel arithmetic of the coil product and of the image half of its adjoint, shared by
// inr_sense.hip, inr_sense_calib.hip and inr_sense_nufft.hip so that the three agree bit for bit.
// Every line is one correctly rounded fp32 operation: contraction is switched off from here to the end of the
// translation unit (the including files switch it off themselves as well).  Unnamed namespace: a copy per unit.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace inr {

namespace {

// x = scale * S * I
__device__ __forceinline__ void apply_one(float ir, float ii, float sr, float si, float scale, float& xr, float& xi) {
  const float a = sr * ir, b = si * ii, c = sr * ii, e = si * ir;
  const float re = a - b, im = c + e;
  xr = scale * re, xi = scale * im;
}

// dI += scale * conj(S) * gX: the operations of inr_sense.hip's grad_one that feed dir / dii, in its order
__device__ __forceinline__ void adjoint_one(float sr, float si, float gr, float gi, float scale, float& dir, float& dii) {
  const float ur = scale * gr, ui = scale * gi;
  const float f = sr * ur, h = si * ui, k = sr * ui, l = si * ur;
  const float tr = f + h, ti = k - l;
  dir = dir + tr, dii = dii + ti;
}

}  // namespace

}  // namespace inr
