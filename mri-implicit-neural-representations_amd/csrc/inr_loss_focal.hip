// inr_loss_focal.hip -- the focal frequency loss (the reference's FocalFrequencyLoss.loss_formulation with matrix = None,
// metrics/losses.py:57-119) on k-space rows out, gt [B,2].  Per sampled row, every fp32 operation rounded
// on its own (contraction is off in this file's arithmetic):
//   e_o = out_o - gt_o      q = e_0 e_0 + e_1 e_1
//   m   = sqrtf(q) (alpha == 1) or powf(sqrtf(q), alpha)          n = logf(m + 1.0f) (log_matrix) or m
//   n_max = max over the sampled rows of n                        (0 when nothing is sampled)
//   w   = 0 if n_max == 0, else fminf(fmaxf(n / n_max, 0), 1)     (a constant of the step: no gradient through it)
//   loss   = ((sum_r w_r q_r) inv) loss_weight
//   dout_o = (((loss_weight 2) e_o) w) inv                        (the product by 2 is exact; w == 1.0f on the row that
//                                                                  attains n_max: focal_n is the one function both passes call)
// Rows with mask == 0: dout = 0, not in n_max, not in the sum.
//
// n_max is a quantity of the whole batch that every row's weight needs, so the loss is no kind of loss_row and takes two
// passes.  Both are streaming kernels in the style of inr_gain.hip: FOCAL_BLOCKS blocks of 256 lanes take contiguous ranges
// of row PAIRS, a lane its pairs lo + lane, lo + lane + 256, ... in order, first row before second; with 16-byte aligned
// out / gt / dout a pair moves as one 16-byte access per array (1 KiB per wave instruction), otherwise the same lane takes
// the same two rows with 8-byte accesses, so no output bit depends on the alignment.  The last row of an odd B is a half pair.
//   pass 1 (focal_max_kernel):  n per sampled row; max per lane, the 256-lane tree, loss_out[FOCAL_MAXIMA + block].
//   pass 2 (focal_grad_kernel): EVERY block folds the FOCAL_BLOCKS maxima itself (lane t holds word t, the same tree; 1 KiB
//       from L2 per block instead of a fold launch between the passes; block 0 stores n_max in loss_out[FOCAL_NMAX]),
//       recomputes e, q, n, writes dout and sums w q in loss_grad_kernel's scheme: a lane's terms in row order, the
//       256-lane tree, loss_out[FOCAL_PARTIALS + block].
//   fold (focal_fold_kernel):   one thread adds the partials in block order and forms loss_out[0].
// Three launches, no atomics: the same inputs give the same bits on every call, and a max does not depend on its order.
// dout == nullptr only drops the stores (validation: the loss alone).
#include "inr_device.h"
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

namespace {

constexpr int FOCAL_THREADS = 256;
static_assert(FOCAL_BLOCKS <= FOCAL_THREADS, "pass 2 folds the maxima with one lane per word");
static_assert(FOCAL_PARTIALS + FOCAL_BLOCKS <= FOCAL_MAXIMA && FOCAL_MAXIMA + FOCAL_BLOCKS <= FOCAL_NMAX && FOCAL_NMAX < 512,
              "the words of loss_out (INR_LOSS_WORDS = 512) overlap");

// e and q of one row
__device__ __forceinline__ float focal_q(float y0, float y1, float t0, float t1, float* e) {
#pragma clang fp contract(off)
  e[0] = y0 - t0;
  e[1] = y1 - t1;
  const float a = e[0] * e[0];
  const float b = e[1] * e[1];
  return a + b;
}

// the weight's numerator of one row: the one definition both passes evaluate
__device__ __forceinline__ float focal_n(const FocalArgs& fa, float q) {
#pragma clang fp contract(off)
  const float r = sqrtf(q);
  const float m = fa.alpha == 1.f ? r : powf(r, fa.alpha);
  return fa.log_matrix ? logf(m + 1.0f) : m;
}

// the two rows of pair p: y, t [4]; the second row of a half pair reads as zeros (and is never live)
template <bool VEC>
__device__ __forceinline__ void focal_load(const float* __restrict__ out, const float* __restrict__ gt, long long r,
                                           bool two, float* yv, float* tv) {
  if (VEC && two) {
    const float4 y4 = *reinterpret_cast<const float4*>(out + 2 * r);
    const float4 t4 = *reinterpret_cast<const float4*>(gt + 2 * r);
    yv[0] = y4.x, yv[1] = y4.y, yv[2] = y4.z, yv[3] = y4.w;
    tv[0] = t4.x, tv[1] = t4.y, tv[2] = t4.z, tv[3] = t4.w;
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool have = j == 0 || two;
      const float2 y2 = have ? reinterpret_cast<const float2*>(out)[r + j] : float2{0.f, 0.f};
      const float2 t2 = have ? reinterpret_cast<const float2*>(gt)[r + j] : float2{0.f, 0.f};
      yv[2 * j] = y2.x, yv[2 * j + 1] = y2.y;
      tv[2 * j] = t2.x, tv[2 * j + 1] = t2.y;
    }
  }
}

// the block's range of row pairs
__device__ __forceinline__ void focal_range(long long B, long long* lo, long long* hi) {
  const long long pairs = (B + 1) >> 1;
  const long long per = (pairs + FOCAL_BLOCKS - 1) / FOCAL_BLOCKS;
  *lo = (long long)blockIdx.x * per;
  if (*lo > pairs) *lo = pairs;
  *hi = *lo + per < pairs ? *lo + per : pairs;
}

template <bool VEC>
__global__ __launch_bounds__(FOCAL_THREADS) void focal_max_kernel(const FocalArgs fa, const float* __restrict__ out,
                                                                  const float* __restrict__ gt,
                                                                  const uint8_t* __restrict__ mask, long long B,
                                                                  float* __restrict__ loss_out) {
  __shared__ float red[FOCAL_THREADS];
  long long lo, hi;
  focal_range(B, &lo, &hi);
  float mx = 0.f;  // n >= 0
  for (long long p = lo + threadIdx.x; p < hi; p += FOCAL_THREADS) {
    const long long r = 2 * p;
    const bool two = r + 1 < B;
    float yv[4], tv[4];
    focal_load<VEC>(out, gt, r, two, yv, tv);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool live = (j == 0 || two) && (mask == nullptr || mask[r + j] != 0);
      if (live) {
        float e[2];
        const float q = focal_q(yv[2 * j], yv[2 * j + 1], tv[2 * j], tv[2 * j + 1], e);
        mx = fmaxf(mx, focal_n(fa, q));
      }
    }
  }
  mx = block_reduce_once<FOCAL_THREADS>(mx, red, MaxF());
  if (threadIdx.x == 0) loss_out[FOCAL_MAXIMA + blockIdx.x] = mx;
}

template <bool VEC, bool GRAD>
__global__ __launch_bounds__(FOCAL_THREADS) void focal_grad_kernel(const FocalArgs fa, const float* __restrict__ out,
                                                                   const float* __restrict__ gt,
                                                                   const uint8_t* __restrict__ mask, long long B,
                                                                   float* loss_out, float* __restrict__ dout) {
  __shared__ float red[FOCAL_THREADS];
  const float n_max = block_reduce<FOCAL_THREADS>(
      threadIdx.x < FOCAL_BLOCKS ? loss_out[FOCAL_MAXIMA + threadIdx.x] : 0.f, red, MaxF());
  if (blockIdx.x == 0 && threadIdx.x == 0) loss_out[FOCAL_NMAX] = n_max;
  const float lw2 = fa.loss_weight * 2.f;  // exact
  long long lo, hi;
  focal_range(B, &lo, &hi);
  float acc = 0.f;
  for (long long p = lo + threadIdx.x; p < hi; p += FOCAL_THREADS) {
    const long long r = 2 * p;
    const bool two = r + 1 < B;
    float yv[4], tv[4], dv[4];
    focal_load<VEC>(out, gt, r, two, yv, tv);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma clang fp contract(off)
      const bool live = (j == 0 || two) && (mask == nullptr || mask[r + j] != 0);
      dv[2 * j] = dv[2 * j + 1] = 0.f;
      if (live) {
        float e[2];
        const float q = focal_q(yv[2 * j], yv[2 * j + 1], tv[2 * j], tv[2 * j + 1], e);
        const float n = focal_n(fa, q);
        const float w = n_max == 0.f ? 0.f : fminf(fmaxf(n / n_max, 0.f), 1.f);
        const float term = w * q;
        acc = acc + term;
        const float c0 = lw2 * e[0];
        const float c1 = lw2 * e[1];
        const float d0 = c0 * w;
        const float d1 = c1 * w;
        dv[2 * j] = d0 * fa.inv_count;
        dv[2 * j + 1] = d1 * fa.inv_count;
      }
    }
    if (GRAD) {
      if (VEC && two) {
        *reinterpret_cast<float4*>(dout + 2 * r) = make_float4(dv[0], dv[1], dv[2], dv[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (j == 0 || two) reinterpret_cast<float2*>(dout)[r + j] = float2{dv[2 * j], dv[2 * j + 1]};
      }
    }
  }
  acc = block_reduce_once<FOCAL_THREADS>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[FOCAL_PARTIALS + blockIdx.x] = acc;
}

// loss_out[0] = ((the partials in block order) inv) loss_weight, by one thread
__global__ void focal_fold_kernel(const FocalArgs fa, float* loss_out) {
#pragma clang fp contract(off)
  float s = 0.f;
  for (int b = 0; b < FOCAL_BLOCKS; ++b) s = s + loss_out[FOCAL_PARTIALS + b];
  const float mean = s * fa.inv_count;
  loss_out[0] = mean * fa.loss_weight;
}

}  // namespace

hipError_t launch_focal_loss_grad(const FocalArgs& fa_in, const float* out, const float* gt, const uint8_t* mask,
                                  long long B, float* loss_out, float* dout, hipStream_t st) {
  FocalArgs fa = fa_in;
  const bool vec_in = (((uintptr_t)out | (uintptr_t)gt) & 15u) == 0;
  const bool vec = vec_in && ((uintptr_t)dout & 15u) == 0;
  hipLaunchKernelGGL(vec_in ? focal_max_kernel<true> : focal_max_kernel<false>, dim3(FOCAL_BLOCKS), dim3(FOCAL_THREADS), 0,
                     st, fa, out, gt, mask, B, loss_out);
  auto* k = dout != nullptr ? (vec ? focal_grad_kernel<true, true> : focal_grad_kernel<false, true>)
                            : (vec ? focal_grad_kernel<true, false> : focal_grad_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(FOCAL_BLOCKS), dim3(FOCAL_THREADS), 0, st, fa, out, gt, mask, B, loss_out, dout);
  hipLaunchKernelGGL(focal_fold_kernel, dim3(1), dim3(1), 0, st, fa, loss_out);
  return hipGetLastError();
}

}  // namespace inr
