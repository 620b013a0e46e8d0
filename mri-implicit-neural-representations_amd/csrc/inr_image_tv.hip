// inr_image_tv.hip -- a total-variation prior on the IMAGE of a SENSE fit (no reference counterpart: the
// reference's tv_loss, inr_tv_grad here, is on a coil's predicted k-space).  img [H][W][2] is one complex image, the image
// network's output of this step.  Smoothed isotropic TV with forward differences that are zero past the last row / column:
//   ax(p) = I[y][x+1] - I[y][x]    ay(p) = I[y+1][x] - I[y][x]                       (complex, component by component)
//   s0 = axr*axr; s1 = axi*axi; s2 = ayr*ayr; s3 = ayi*ayi; a = s0 + s1; b = s2 + s3; q0 = a + b; q = q0 + e2
//   n(p) = sqrtf(q)                       e2 = eps*eps (one fp32 product, on the host)
//   u(p) = ax / n;  v(p) = ay / n         (IEEE division per component; both (0, 0) where n == 0, which needs eps == 0)
//   term(p) = n - eps
//   t0 = u(left of p) - u(p);  t1 = v(above p) - v(p);  t = t0 + t1;  d(p) = c * t      (a missing neighbour's u / v is 0)
//   dimg[p] = d(p)  or  dimg[p] + d(p)    c = fl(weight / (H W)), formed in fp64 on the host and rounded once
//   loss_out[0] = fl(S * (weight / (H W)))    S = the fp64 sum of the fp32 terms, the product in fp64, rounded once
// Every line of the fp32 chain is one correctly rounded operation (contraction is switched off for this file, as in
// inr_sense.hip); inr_mi355x/sense_prior.py (image_tv_numpy) is the same text in numpy, bit for bit in dimg.
//
// Mapping: a gather.  One lane owns its pixel -- or, where W is even, two neighbouring pixels (x, x + 1), x even, moved as
// one 16-byte access when every pointer is 16-byte aligned and as two of 8 bytes otherwise -- and recomputes n at its own
// pixel, at its left and at its upper neighbour from a 7-point read stencil (the image is 1.9 MB at 640 x 368 and stays
// in L2): no atomics, no LDS tile, the same bits on every call and on either path.  TV_THREADS lanes per block,
// grid-strided beyond TV_BLOCKS.
// The value: a lane adds its terms in fp64 in the order it meets them, the block folds the lanes with inr_reduce.h's
// fixed tree and stores one fp64 partial at loss_out[IMAGE_TV_PARTIALS + 2 block]; a second launch of one thread adds
// the partials in block order.  dimg == nullptr drops the neighbours and the stores (validation: the value alone).
#include <hip/hip_runtime.h>
#include "inr_aux.h"
#include "inr_reduce.h"

#pragma clang fp contract(off)

namespace inr {

namespace {

constexpr int TV_THREADS = IMAGE_TV_THREADS;
constexpr int TV_BLOCKS = IMAGE_TV_BLOCKS;

struct TvDims {
  long long H, W;
  long long row_units;  // W, or W / 2 on the pair path
  long long units;      // H * row_units
  float eps, e2, c;
};

struct TvCell {
  float n, ur, ui, vr, vi;
};

// n, u, v of the pixel whose value is c, from its right (r) and lower (d) neighbours where it has them
__device__ __forceinline__ TvCell tv_cell(float2 c, float2 r, float2 d, bool has_r, bool has_d, float e2) {
  const float axr = has_r ? r.x - c.x : 0.f, axi = has_r ? r.y - c.y : 0.f;
  const float ayr = has_d ? d.x - c.x : 0.f, ayi = has_d ? d.y - c.y : 0.f;
  const float s0 = axr * axr, s1 = axi * axi, s2 = ayr * ayr, s3 = ayi * ayi;
  const float a = s0 + s1, b = s2 + s3;
  const float q0 = a + b;
  const float q = q0 + e2;
  TvCell o;
  o.n = sqrtf(q);
  if (o.n > 0.f) {
    o.ur = axr / o.n, o.ui = axi / o.n;
    o.vr = ayr / o.n, o.vi = ayi / o.n;
  } else {
    o.ur = o.ui = o.vr = o.vi = 0.f;
  }
  return o;
}

// d(p) of the pixel with cell P, from its left neighbour's u and its upper neighbour's v
__device__ __forceinline__ float2 tv_grad(const TvCell& P, float ulr, float uli, float vur, float vui, float c) {
  const float t0r = ulr - P.ur, t0i = uli - P.ui;
  const float t1r = vur - P.vr, t1i = vui - P.vi;
  const float tr = t0r + t1r, ti = t0i + t1i;
  return make_float2(c * tr, c * ti);
}

__device__ __forceinline__ void tv_row_of(const TvDims& d, long long u, long long* y, long long* xu) {
  if (d.units <= 0xffffffffLL) {  // uniform: the 32-bit division is several times cheaper
    const unsigned uu = (unsigned)u, w = (unsigned)d.row_units;
    const unsigned yy = uu / w;
    *y = yy, *xu = uu - yy * w;
  } else {
    *y = u / d.row_units, *xu = u - *y * d.row_units;
  }
}

// two neighbouring pixels: one 16-byte access (VEC), or two of 8 bytes
template <bool VEC>
__device__ __forceinline__ float4 tv_load2(const float2* q) {
  if constexpr (VEC) return *reinterpret_cast<const float4*>(q);
  const float2 a = q[0], b = q[1];
  return make_float4(a.x, a.y, b.x, b.y);
}

template <bool VEC>
__device__ __forceinline__ void tv_store2(float2* q, float4 v) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(q) = v;
  } else {
    q[0] = make_float2(v.x, v.y), q[1] = make_float2(v.z, v.w);
  }
}

// PAIR (W even): a unit is the pixels (x, x + 1), x even, whatever the alignment -- the lanes, and with them the order of
// the fp64 sum, do not depend on it; VEC (every pointer 16-byte aligned) only widens the accesses
template <bool PAIR, bool VEC, bool GRAD, bool ACC>
__global__ __launch_bounds__(TV_THREADS) void image_tv_kernel(const float* __restrict__ img, float* __restrict__ dimg,
                                                              const TvDims d, float* __restrict__ loss_out) {
  __shared__ double red[TV_THREADS];
  const float2* I = reinterpret_cast<const float2*>(img);
  const float2 zero = make_float2(0.f, 0.f);
  double sum = 0.0;
  for (long long u = (long long)blockIdx.x * TV_THREADS + threadIdx.x; u < d.units; u += (long long)gridDim.x * TV_THREADS) {
    long long y, xu;
    tv_row_of(d, u, &y, &xu);
    const bool has_d = y + 1 < d.H, has_up = y > 0;
    if constexpr (PAIR) {
      const long long x = 2 * xu;             // x + 1 < W: W is even
      const long long p = y * d.W + x;        // even: a 16-byte boundary under VEC
      const bool has_r2 = x + 2 < d.W, has_l = x > 0;
      const float4 c4 = tv_load2<VEC>(I + p);
      const float2 c0 = make_float2(c4.x, c4.y), c1 = make_float2(c4.z, c4.w);
      const float2 r2 = has_r2 ? I[p + 2] : zero;
      float2 d0 = zero, d1 = zero;
      if (has_d) {
        const float4 d4 = tv_load2<VEC>(I + p + d.W);
        d0 = make_float2(d4.x, d4.y), d1 = make_float2(d4.z, d4.w);
      }
      const TvCell P0 = tv_cell(c0, c1, d0, true, has_d, d.e2);
      const TvCell P1 = tv_cell(c1, r2, d1, has_r2, has_d, d.e2);
      const float term0 = P0.n - d.eps, term1 = P1.n - d.eps;
      sum += (double)term0;
      sum += (double)term1;
      if constexpr (GRAD) {
        float ulr = 0.f, uli = 0.f;
        if (has_l) {
          const TvCell Lc = tv_cell(I[p - 1], c0, has_d ? I[p - 1 + d.W] : zero, true, has_d, d.e2);
          ulr = Lc.ur, uli = Lc.ui;
        }
        float v0r = 0.f, v0i = 0.f, v1r = 0.f, v1i = 0.f;
        if (has_up) {
          const float4 u4 = tv_load2<VEC>(I + p - d.W);
          const float2 u0 = make_float2(u4.x, u4.y), u1 = make_float2(u4.z, u4.w);
          const float2 ur2 = has_r2 ? I[p - d.W + 2] : zero;
          const TvCell U0 = tv_cell(u0, u1, c0, true, true, d.e2);
          const TvCell U1 = tv_cell(u1, ur2, c1, has_r2, true, d.e2);
          v0r = U0.vr, v0i = U0.vi, v1r = U1.vr, v1i = U1.vi;
        }
        const float2 g0 = tv_grad(P0, ulr, uli, v0r, v0i, d.c);
        const float2 g1 = tv_grad(P1, P0.ur, P0.ui, v1r, v1i, d.c);
        float4 o = make_float4(g0.x, g0.y, g1.x, g1.y);
        float2* out = reinterpret_cast<float2*>(dimg) + p;
        if constexpr (ACC) {
          const float4 was = tv_load2<VEC>(out);
          o.x = was.x + o.x, o.y = was.y + o.y, o.z = was.z + o.z, o.w = was.w + o.w;
        }
        tv_store2<VEC>(out, o);
      }
    } else {
      const long long x = xu;
      const long long p = y * d.W + x;
      const bool has_r = x + 1 < d.W, has_l = x > 0;
      const float2 c = I[p];
      const float2 r = has_r ? I[p + 1] : zero;
      const float2 dn = has_d ? I[p + d.W] : zero;
      const TvCell P = tv_cell(c, r, dn, has_r, has_d, d.e2);
      const float term = P.n - d.eps;
      sum += (double)term;
      if constexpr (GRAD) {
        float ulr = 0.f, uli = 0.f, vur = 0.f, vui = 0.f;
        if (has_l) {
          const TvCell Lc = tv_cell(I[p - 1], c, has_d ? I[p - 1 + d.W] : zero, true, has_d, d.e2);
          ulr = Lc.ur, uli = Lc.ui;
        }
        if (has_up) {
          const TvCell Uc = tv_cell(I[p - d.W], has_r ? I[p - d.W + 1] : zero, c, has_r, true, d.e2);
          vur = Uc.vr, vui = Uc.vi;
        }
        float2 o = tv_grad(P, ulr, uli, vur, vui, d.c);
        float2* out = reinterpret_cast<float2*>(dimg) + p;
        if constexpr (ACC) {
          const float2 was = *out;
          o.x = was.x + o.x, o.y = was.y + o.y;
        }
        *out = o;
      }
    }
  }
  sum = block_reduce_once<TV_THREADS>(sum, red, Sum());
  if (threadIdx.x == 0) reinterpret_cast<double*>(loss_out + IMAGE_TV_PARTIALS)[blockIdx.x] = sum;
}

// loss_out[0] = fl((the partials in block order) * scale), by one thread
__global__ void image_tv_fold_kernel(float* loss_out, int blocks, double scale) {
  const double* part = reinterpret_cast<const double*>(loss_out + IMAGE_TV_PARTIALS);
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s = s + part[b];
  loss_out[0] = (float)(s * scale);
}

template <bool PAIR, bool VEC>
auto* tv_pick(bool grad, bool acc) {
  return !grad ? image_tv_kernel<PAIR, VEC, false, false>
               : acc ? image_tv_kernel<PAIR, VEC, true, true> : image_tv_kernel<PAIR, VEC, true, false>;
}

}  // namespace

hipError_t launch_image_tv_grad(const float* img, long long H, long long W, float weight, float eps, bool accumulate,
                                float* loss_out, float* dimg, hipStream_t st) {
  const bool pair = W % 2 == 0;
  const bool vec = pair && (((uintptr_t)img | (uintptr_t)dimg) & 15u) == 0;  // a null dimg is aligned
  TvDims d;
  d.H = H, d.W = W;
  d.row_units = pair ? W / 2 : W;
  d.units = H * d.row_units;
  d.eps = eps;
  d.e2 = eps * eps;
  const double scale = (double)weight / (double)(H * W);
  d.c = (float)scale;
  const long long nb = (d.units + TV_THREADS - 1) / TV_THREADS;
  const int blocks = (int)(nb < TV_BLOCKS ? nb : TV_BLOCKS);
  const bool grad = dimg != nullptr;
  auto* k = vec ? tv_pick<true, true>(grad, accumulate) : pair ? tv_pick<true, false>(grad, accumulate)
                                                                : tv_pick<false, false>(grad, accumulate);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(TV_THREADS), 0, st, img, dimg, d, loss_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(image_tv_fold_kernel, dim3(1), dim3(1), 0, st, loss_out, blocks, scale);
  return hipGetLastError();
}

}  // namespace inr
