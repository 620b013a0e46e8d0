// inr_gain.hip -- the operation that joins a backbone and a learned radial-gain network (the reference's ScalerWrapper,
// models/networks.py:380-405): per row, with y [B,2] the backbone's output and s [B] the gain network's,
//   g     = expf(-s)
//   res_c = y_c * g                                   (written for every row when `res` is given)
//   (loss, dres) = loss_row(ld, 2, res, gt)           (csrc/inr_device.h: the function inr_loss_grad calls)
//   dy_c  = dres_c * g
//   ds    = -(dres_0 * res_0 + dres_1 * res_1)
// Rows with mask == 0 never reach loss_row: dy = ds = 0, nothing added to the loss.
//
// Mapping: a streaming kernel, 41 bytes per row with res (33 without).  Rows are 8-byte (re, im) pairs, so a lane takes
// TWO consecutive rows: y, gt, dy and res move as one 16-byte access each, s and ds as one 8-byte access, consecutive
// lanes at consecutive addresses (1 KiB per wave instruction on the four wide arrays).  GAIN_BLOCKS blocks of 256 lanes
// take contiguous ranges of row pairs, a lane its pairs lo + lane, lo + lane + 256, ... in order, first row before second.
// The wide accesses need y, gt, dy, res 16-byte and s, ds 8-byte aligned (VEC); otherwise the same lane takes the same two
// rows with 8- and 4-byte accesses, so the bits of every output do not depend on the alignment.  The last row of an odd B
// is a half pair.
//
// The loss sum follows loss_grad_kernel's scheme (inr_loss.hip): a lane's terms in row order, the fixed 256-lane tree,
// ordered partials in loss_out[1 .. GAIN_BLOCKS], then one thread folds them in block order.  No atomics: the same
// inputs give the same bits on every call.
#include "inr_device.h"
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

namespace {

constexpr int GAIN_THREADS = 256;
constexpr int GAIN_BLOCKS = 256;     // partials in loss_out[1 .. 256]: INR_LOSS_WORDS = 512 holds them
constexpr int GAIN_APPLY_MAX_BLOCKS = 2048;

// one row: everything the kernel computes for it.  `live`: the row enters the loss
__device__ __forceinline__ float gain_row(const LossDesc& ld, bool live, float y0, float y1, float s, float t0, float t1,
                                          float* res, float* dy, float* ds) {
  // no contraction of these products into loss_row's sums: res is the rounded product whether or not it is stored, so
  // res == NULL changes no bit of dy, ds or the loss, and inr_gain_apply's res equals this one
#pragma clang fp contract(off)
  const float g = expf(-s);
  res[0] = y0 * g;
  res[1] = y1 * g;
  dy[0] = dy[1] = 0.f;
  *ds = 0.f;
  if (!live) return 0.f;
  const float t[2] = {t0, t1};
  float dres[2] = {0.f, 0.f};
  const float loss = loss_row(ld, 2, res, t, dres);
  dy[0] = dres[0] * g;
  dy[1] = dres[1] * g;
  *ds = -(dres[0] * res[0] + dres[1] * res[1]);
  return loss;
}

template <bool VEC, bool RES>
__global__ __launch_bounds__(GAIN_THREADS) void gain_loss_grad_kernel(const LossDesc ld, const float* __restrict__ y,
                                                                      const float* __restrict__ s,
                                                                      const float* __restrict__ gt,
                                                                      const uint8_t* __restrict__ mask, long long B,
                                                                      float* __restrict__ res, float* __restrict__ loss_out,
                                                                      float* __restrict__ dy, float* __restrict__ ds) {
  __shared__ float red[GAIN_THREADS];
  const long long pairs = (B + 1) >> 1;
  const long long per = (pairs + GAIN_BLOCKS - 1) / GAIN_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < pairs ? lo + per : pairs;
  float acc = 0.f;
  for (long long p = lo + threadIdx.x; p < hi; p += GAIN_THREADS) {
    const long long r = 2 * p;
    const bool two = r + 1 < B;  // false only for the last row of an odd B
    float yv[4], tv[4], sv[2];
    if (VEC && two) {
      const float4 y4 = *reinterpret_cast<const float4*>(y + 2 * r);
      const float4 t4 = *reinterpret_cast<const float4*>(gt + 2 * r);
      const float2 s2 = *reinterpret_cast<const float2*>(s + r);
      yv[0] = y4.x, yv[1] = y4.y, yv[2] = y4.z, yv[3] = y4.w;
      tv[0] = t4.x, tv[1] = t4.y, tv[2] = t4.z, tv[3] = t4.w;
      sv[0] = s2.x, sv[1] = s2.y;
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool have = j == 0 || two;
        const float2 y2 = have ? reinterpret_cast<const float2*>(y)[r + j] : float2{0.f, 0.f};
        const float2 t2 = have ? reinterpret_cast<const float2*>(gt)[r + j] : float2{0.f, 0.f};
        yv[2 * j] = y2.x, yv[2 * j + 1] = y2.y;
        tv[2 * j] = t2.x, tv[2 * j + 1] = t2.y;
        sv[j] = have ? s[r + j] : 0.f;
      }
    }
    float rv[4], dv[4], dsv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool have = j == 0 || two;
      const bool live = have && (mask == nullptr || mask[r + j] != 0);
      acc += gain_row(ld, live, yv[2 * j], yv[2 * j + 1], sv[j], tv[2 * j], tv[2 * j + 1], rv + 2 * j, dv + 2 * j, dsv + j);
    }
    if (VEC && two) {
      *reinterpret_cast<float4*>(dy + 2 * r) = make_float4(dv[0], dv[1], dv[2], dv[3]);
      *reinterpret_cast<float2*>(ds + r) = float2{dsv[0], dsv[1]};
      if (RES) *reinterpret_cast<float4*>(res + 2 * r) = make_float4(rv[0], rv[1], rv[2], rv[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (j == 0 || two) {
          reinterpret_cast<float2*>(dy)[r + j] = float2{dv[2 * j], dv[2 * j + 1]};
          ds[r + j] = dsv[j];
          if (RES) reinterpret_cast<float2*>(res)[r + j] = float2{rv[2 * j], rv[2 * j + 1]};
        }
    }
  }
  acc = block_reduce_once<GAIN_THREADS>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[1 + blockIdx.x] = acc;
}

// loss_out[0] = the partials in block order, by one thread (loss_fold_kernel's scheme over GAIN_BLOCKS words)
__global__ void gain_fold_kernel(float* loss_out) {
  float s = 0.f;
  for (int b = 0; b < GAIN_BLOCKS; ++b) s += loss_out[1 + b];
  loss_out[0] = s;
}

// res = y * expf(-s): the same two operations as gain_row, so the bits equal inr_gain_loss_grad's res.  A lane reads its
// rows before it writes them and touches no other lane's, so res == y is allowed (no __restrict__ on the two)
template <bool VEC>
__global__ __launch_bounds__(GAIN_THREADS) void gain_apply_kernel(const float* y, const float* __restrict__ s, long long B,
                                                                  float* res) {
  const long long pairs = (B + 1) >> 1;
  for (long long p = (long long)blockIdx.x * GAIN_THREADS + threadIdx.x; p < pairs; p += (long long)gridDim.x * GAIN_THREADS) {
    const long long r = 2 * p;
    if (VEC && r + 1 < B) {
      const float4 y4 = *reinterpret_cast<const float4*>(y + 2 * r);
      const float2 s2 = *reinterpret_cast<const float2*>(s + r);
      const float g0 = expf(-s2.x), g1 = expf(-s2.y);
      *reinterpret_cast<float4*>(res + 2 * r) = make_float4(y4.x * g0, y4.y * g0, y4.z * g1, y4.w * g1);
    } else {
      for (long long q = r; q < r + 2 && q < B; ++q) {
        const float2 y2 = reinterpret_cast<const float2*>(y)[q];
        const float g = expf(-s[q]);
        reinterpret_cast<float2*>(res)[q] = float2{y2.x * g, y2.y * g};
      }
    }
  }
}

}  // namespace

hipError_t launch_gain_loss_grad(const LossDesc& ld_in, const float* y, const float* s, const float* gt,
                                 const uint8_t* mask, long long B, float* res, float* loss_out, float* dy, float* ds,
                                 hipStream_t st) {
  LossDesc ld = ld_in;
  const bool vec = (((uintptr_t)y | (uintptr_t)gt | (uintptr_t)dy | (uintptr_t)res) & 15u) == 0 &&
                   (((uintptr_t)s | (uintptr_t)ds) & 7u) == 0;
  auto* k = vec ? (res ? gain_loss_grad_kernel<true, true> : gain_loss_grad_kernel<true, false>)
                : (res ? gain_loss_grad_kernel<false, true> : gain_loss_grad_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(GAIN_BLOCKS), dim3(GAIN_THREADS), 0, st, ld, y, s, gt, mask, B, res, loss_out, dy, ds);
  hipLaunchKernelGGL(gain_fold_kernel, dim3(1), dim3(1), 0, st, loss_out);
  return hipGetLastError();
}

hipError_t launch_gain_apply(const float* y, const float* s, long long B, float* res, hipStream_t st) {
  const long long pairs = (B + 1) >> 1;
  const long long want = (pairs + GAIN_THREADS - 1) / GAIN_THREADS;
  const unsigned blocks = (unsigned)(want < GAIN_APPLY_MAX_BLOCKS ? want : GAIN_APPLY_MAX_BLOCKS);
  const bool vec = (((uintptr_t)y | (uintptr_t)res) & 15u) == 0 && ((uintptr_t)s & 7u) == 0;
  hipLaunchKernelGGL(vec ? gain_apply_kernel<true> : gain_apply_kernel<false>, dim3(blocks), dim3(GAIN_THREADS), 0, st, y, s,
                     B, res);
  return hipGetLastError();
}

}  // namespace inr
