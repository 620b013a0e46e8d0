// inr_loss.hip -- losses on the network output and their gradients (gfx950): pointwise, multi-head, total variation,
// loss + TV in one pass, CenterLoss pairs.  HBM-bound streaming kernels; every sum runs in a fixed order.
#include "inr_device.h"
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

// ---------------------------------------------------------------------------------------------
// Pointwise losses + their gradient w.r.t. the network output (tier 1; metrics/losses.py and
// train.py:172-182).  64 blocks write ordered partial sums to loss_out[1..64]; a single thread
// then folds them into loss_out[0] (deterministic).
// ---------------------------------------------------------------------------------------------
#define LOSS_BLOCKS 64

__global__ __launch_bounds__(256) void loss_grad_kernel(const LossDesc ld, const float* __restrict__ out,
                                                        const float* __restrict__ gt,
                                                        const uint8_t* __restrict__ mask, long long B,
                                                        float* __restrict__ loss_out, float* __restrict__ dout) {
  __shared__ float red[256];
  // contiguous row range per block, rows visited in order by a fixed thread -> fixed sum order
  const long long per = (B + LOSS_BLOCKS - 1) / LOSS_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < B ? lo + per : B;
  float acc = 0.f;
  for (long long r = lo + threadIdx.x; r < hi; r += 256) {
    float g[2] = {0.f, 0.f};
    if (mask == nullptr || mask[r] != 0) {
      const float y[2] = {out[2 * r], out[2 * r + 1]};
      const float t[2] = {gt[2 * r], gt[2 * r + 1]};
      acc += loss_row(ld, 2, y, t, g);
    }
    dout[2 * r] = g[0];
    dout[2 * r + 1] = g[1];
  }
  acc = block_reduce_once<256>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[1 + blockIdx.x] = acc;
}

// loss_out[0] = (ADD: +=) the partials in block order, by one thread
template <bool ADD>
__global__ void loss_fold_kernel(float* loss_out) {
  float s = 0.f;
  for (int b = 0; b < LOSS_BLOCKS; ++b) s += loss_out[1 + b];
  loss_out[0] = ADD ? loss_out[0] + s : s;
}

hipError_t launch_loss_grad(const LossDesc& ld_in, const float* out, const float* gt, const uint8_t* mask, long long B,
                            float* loss_out, float* dout, hipStream_t st) {
  LossDesc ld = ld_in;
  hipLaunchKernelGGL(loss_grad_kernel, dim3(LOSS_BLOCKS), dim3(256), 0, st, ld, out, gt, mask, B, loss_out, dout);
  hipLaunchKernelGGL(loss_fold_kernel<false>, dim3(1), dim3(1), 0, st, loss_out);
  return hipGetLastError();
}

// Multi-head version (tier 1 of the multiscale loop, train_kspace_multiscale.py:176-195): outs / douts [NH][B][2],
// pointwise terms on sampled rows, ConsistencyLoss on every row (mfn_loss_row).
__global__ __launch_bounds__(256) void loss_grad_multi_kernel(const LossDesc ld, const float* __restrict__ outs,
                                                              const float* __restrict__ gt,
                                                              const float* __restrict__ dist,
                                                              const uint8_t* __restrict__ mask, int NH, long long B,
                                                              float* __restrict__ loss_out, float* __restrict__ douts) {
  __shared__ float red[256];
  const long long per = (B + LOSS_BLOCKS - 1) / LOSS_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < B ? lo + per : B;
  float acc = 0.f;
  for (long long r = lo + threadIdx.x; r < hi; r += 256) {
    float y[INR_MAX_HEADS][4], g[INR_MAX_HEADS][4];
#pragma unroll
    for (int k = 0; k < INR_MAX_HEADS; ++k)
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        y[k][o] = (k < NH && o < 2) ? outs[((size_t)k * B + r) * 2 + o] : 0.f;
        g[k][o] = 0.f;
      }
    const float t[4] = {gt[2 * r], gt[2 * r + 1], 0.f, 0.f};
    acc += mfn_loss_row(ld, NH, 2, y, t, dist != nullptr ? dist[r] : 0.f, g, mask == nullptr || mask[r] != 0);
#pragma unroll
    for (int k = 0; k < INR_MAX_HEADS; ++k)
      if (k < NH) {
        douts[((size_t)k * B + r) * 2] = g[k][0];
        douts[((size_t)k * B + r) * 2 + 1] = g[k][1];
      }
  }
  acc = block_reduce_once<256>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[1 + blockIdx.x] = acc;
}

hipError_t launch_loss_grad_multi(const LossDesc& ld_in, const float* outs, const float* gt, const float* dist,
                                  const uint8_t* mask, int NH, long long B, float* loss_out, float* douts,
                                  hipStream_t st) {
  LossDesc ld = ld_in;
  hipLaunchKernelGGL(loss_grad_multi_kernel, dim3(LOSS_BLOCKS), dim3(256), 0, st, ld, outs, gt, dist, mask, NH, B,
                     loss_out, douts);
  hipLaunchKernelGGL(loss_fold_kernel<false>, dim3(1), dim3(1), 0, st, loss_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Total-variation regulariser on one coil's predicted k-space image (metrics/losses.py tv_loss;
// train.py:172-175):  w * ( mean|img[:, :-1] - img[:, 1:]| + mean|img[:-1] - img[1:]| ) over
// img [H][W][2].  `out` holds rows [y0, y0 + R) of the image; the first R_own rows are this
// caller's (a trailing halo row lets the vertical pair (y0+R_own-1, y0+R_own) be evaluated by the
// rank that owns its upper row).  Gather form: every element sums the sign terms of the <= 4 pairs
// it belongs to, so there are no atomics and the result is deterministic.  Adds into dout and
// loss_out[0].
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void tv_grad_kernel(const float* __restrict__ out, long long R, long long R_own,
                                                      long long W, float cw, float ch,
                                                      float* __restrict__ loss_out, float* __restrict__ dout) {
  __shared__ float red[256];
  const long long n = R * W * 2;
  const long long per = (n + LOSS_BLOCKS - 1) / LOSS_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < n ? lo + per : n;
  const long long rs = W * 2;  // row stride
  float acc = 0.f;
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const long long r = i / rs;
    const long long x = (i - r * rs) >> 1;
    const float v = out[i];
    float g = 0.f;
    if (r < R_own) {
      if (x + 1 < W) {
        const float d = v - out[i + 2];
        acc += fabsf(d) * cw;
        g += cw * sgn(d);
      }
      if (x > 0) g -= cw * sgn(out[i - 2] - v);
      if (r + 1 < R) {
        const float d = v - out[i + rs];
        acc += fabsf(d) * ch;
        g += ch * sgn(d);
      }
    }
    if (r > 0 && r - 1 < R_own) g -= ch * sgn(out[i - rs] - v);
    dout[i] += g;
  }
  acc = block_reduce_once<256>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[1 + blockIdx.x] = acc;
}

hipError_t launch_tv_grad(const float* out, long long R, long long R_own, long long W, float cw, float ch,
                          float* loss_out, float* dout, hipStream_t st) {
  hipLaunchKernelGGL(tv_grad_kernel, dim3(LOSS_BLOCKS), dim3(256), 0, st, out, R, R_own, W, cw, ch, loss_out, dout);
  hipLaunchKernelGGL(loss_fold_kernel<true>, dim3(1), dim3(1), 0, st, loss_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// inr_loss_grad + inr_tv_grad of one coil's rows in ONE pass (the per-coil step of train.py:163-189 with use_tv): a thread
// per coordinate, 256 workgroups over the R x W grid (the two kernels above are 64 workgroups each for 6 MB of traffic:
// 18 + 40 us of a 0.58 ms step, plus two single-thread folds and the copy that zeroed the halo rows' mask).  Pointwise loss
// on the sampled rows the caller OWNS (r < R_own: a data-parallel rank's halo row below its slab stays with its owner),
// TV as tv_grad_kernel.  dout is WRITTEN (not added to).  Partial sums: loss_out[1 + block], fixed order within a thread
// (its coordinates in order), fixed tree within a block; loss_tv_fold_kernel sums the 256 partials by a fixed tree.
// ---------------------------------------------------------------------------------------------
#define LOSS_TV_BLOCKS 256

__global__ __launch_bounds__(256) void loss_tv_grad_kernel(const LossDesc ld, const float* __restrict__ out,
                                                           const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                           long long R, long long R_own, long long W, float cw, float ch,
                                                           float* __restrict__ loss_out, float* __restrict__ dout) {
  __shared__ float red[256];
  const long long n = R * W;
  const long long per = (n + LOSS_TV_BLOCKS - 1) / LOSS_TV_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < n ? lo + per : n;
  const float2* __restrict__ o2 = reinterpret_cast<const float2*>(out);
  float acc = 0.f;
  for (long long c = lo + threadIdx.x; c < hi; c += 256) {
    const long long r = c / W, x = c - r * W;
    const float2 v = o2[c];
    float g[2] = {0.f, 0.f};
    if (r < R_own && (mask == nullptr || mask[c] != 0)) {
      const float y[2] = {v.x, v.y};
      const float2 tt = reinterpret_cast<const float2*>(gt)[c];
      const float t[2] = {tt.x, tt.y};
      acc += loss_row(ld, 2, y, t, g);
    }
    if (r < R_own) {
      if (x + 1 < W) {
        const float2 e = o2[c + 1];
        const float d0 = v.x - e.x, d1 = v.y - e.y;
        acc += (fabsf(d0) + fabsf(d1)) * cw;
        g[0] += cw * sgn(d0);
        g[1] += cw * sgn(d1);
      }
      if (x > 0) {
        const float2 e = o2[c - 1];
        g[0] -= cw * sgn(e.x - v.x);
        g[1] -= cw * sgn(e.y - v.y);
      }
      if (r + 1 < R) {
        const float2 e = o2[c + W];
        const float d0 = v.x - e.x, d1 = v.y - e.y;
        acc += (fabsf(d0) + fabsf(d1)) * ch;
        g[0] += ch * sgn(d0);
        g[1] += ch * sgn(d1);
      }
    }
    if (r > 0 && r - 1 < R_own) {
      const float2 e = o2[c - W];
      g[0] -= ch * sgn(e.x - v.x);
      g[1] -= ch * sgn(e.y - v.y);
    }
    reinterpret_cast<float2*>(dout)[c] = float2{g[0], g[1]};
  }
  acc = block_reduce_once<256>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[1 + blockIdx.x] = acc;
}

// a tree over the 256 partials, not their sum in order: not loss_fold_kernel
__global__ __launch_bounds__(256) void loss_tv_fold_kernel(float* loss_out) {
  __shared__ float red[256];
  const float s = block_reduce_once<256>(loss_out[1 + threadIdx.x], red, Sum());
  if (threadIdx.x == 0) loss_out[0] = s;
}

hipError_t launch_loss_tv_grad(const LossDesc& ld_in, const float* out, const float* gt, const uint8_t* mask, long long R,
                               long long R_own, long long W, float cw, float ch, float* loss_out, float* dout,
                               hipStream_t st) {
  LossDesc ld = ld_in;
  hipLaunchKernelGGL(loss_tv_grad_kernel, dim3(LOSS_TV_BLOCKS), dim3(256), 0, st, ld, out, gt, mask, R, R_own, W, cw, ch,
                     loss_out, dout);
  hipLaunchKernelGGL(loss_tv_fold_kernel, dim3(1), dim3(256), 0, st, loss_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// CenterLoss, random-pair term of one band (metrics/losses.py:175-199): for pairs p < n of rows (a_p, b_p) -- drawn by the
// caller with torch.randperm exactly as the reference draws them -- r_p = (|t_a| - |t_b|) - (|y_a| - |y_b|), the band adds
// w * sum_p r_p^2 (w = 0.1 / n) to the loss and  -2 w r_p y_a / |y_a|  to dout[a_p],  +2 w r_p y_b / |y_b|  to dout[b_p].
// The a rows of a band are distinct, so are the b rows, and no row is in both (they come from disjoint radial masks): plain
// read-modify-write, no atomics; bands are separate launches on one stream.  Rows outside [0, B) are ignored.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void center_pairs_kernel(const float* __restrict__ out, const float* __restrict__ gt,
                                                           const long long* __restrict__ ia, const long long* __restrict__ ib,
                                                           long long n, long long B, float w, float* __restrict__ loss_out,
                                                           float* __restrict__ dout) {
  __shared__ float red[256];
  const long long per = (n + LOSS_BLOCKS - 1) / LOSS_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < n ? lo + per : n;
  float acc = 0.f;
  for (long long p = lo + threadIdx.x; p < hi; p += 256) {
    const long long a = ia[p], b = ib[p];
    if (a < 0 || a >= B || b < 0 || b >= B) continue;
    const float yar = out[2 * a], yai = out[2 * a + 1], ybr = out[2 * b], ybi = out[2 * b + 1];
    const float na = sqrtf(yar * yar + yai * yai), nb = sqrtf(ybr * ybr + ybi * ybi);
    const float ta = sqrtf(gt[2 * a] * gt[2 * a] + gt[2 * a + 1] * gt[2 * a + 1]);
    const float tb = sqrtf(gt[2 * b] * gt[2 * b] + gt[2 * b + 1] * gt[2 * b + 1]);
    const float r = (ta - tb) - (na - nb);
    acc += w * r * r;
    const float ca = na > 0.f ? -2.f * w * r / na : 0.f;  // d|y|/dy = y / |y| (0 at the origin, as torch.abs)
    const float cb = nb > 0.f ? 2.f * w * r / nb : 0.f;
    dout[2 * a] += ca * yar;
    dout[2 * a + 1] += ca * yai;
    dout[2 * b] += cb * ybr;
    dout[2 * b + 1] += cb * ybi;
  }
  acc = block_reduce_once<256>(acc, red, Sum());
  if (threadIdx.x == 0) loss_out[1 + blockIdx.x] = acc;
}

hipError_t launch_center_pairs(const float* out, const float* gt, const long long* ia, const long long* ib, long long n,
                               long long B, float w, float* loss_out, float* dout, hipStream_t st) {
  hipLaunchKernelGGL(center_pairs_kernel, dim3(LOSS_BLOCKS), dim3(256), 0, st, out, gt, ia, ib, n, B, w, loss_out, dout);
  hipLaunchKernelGGL(loss_fold_kernel<true>, dim3(1), dim3(1), 0, st, loss_out);
  return hipGetLastError();
}

}  // namespace inr
