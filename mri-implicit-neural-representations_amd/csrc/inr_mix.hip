// inr_mix.hip -- the operation that joins K expert networks and a gate network (the reference's MultiHeadWrapper with
// backbone = None, models/networks.py:275-328): per row, with y_k [B,2] expert k's output, w [B,K] the
// gate's, d the row's k-space radius, t the target,
//   pre_c = sum_k w_k y_kc                       (head order; every product and sum rounded on its own)
//   res_c = clamp ? min(max(pre_c, -1), 1) : pre_c         (written for every row when `res` is given)
//   (L_0, dres) = loss_row(ld | inv_count[0], res, t)
//   dpre_c = dres_c where !clamp or -1 <= pre_c <= 1 (both ends included, as torch.clamp), else 0
//   dw_k   = dpre_0 y_k0 + dpre_1 y_k1
//   ring k (radii[k] <= d <= radii[k+1], both ends included):  (L_{1+k}, g_k) = loss_row(ld | inv_count[1+k], y_k, t)
//   dy_kc  = g_kc (0 off the ring)  [+ w_k dpre_c  when !detach]
// Rows with mask == 0 never reach loss_row: dy = dw = 0, nothing added to any term.
//
// Mapping: a streaming kernel, 8 (2K + 2) + 8K + 5 bytes per row with res (117 at K = 4).  As in inr_gain.hip a lane
// takes TWO consecutive rows: every [B,2] array (y_k, dy_k, gt, res) moves as one 16-byte access, dist as one 8-byte
// access, and the lane's 2K gate weights -- contiguous in the row-major [B,K] arrays -- as K/2 16-byte (K even) or K
// 8-byte (K odd) accesses, consecutive lanes at consecutive 8K-byte pieces, so a wave's accesses to w and dw cover one
// contiguous 512 K-byte range.  K is a template parameter (the launcher dispatches on n_heads): the per-head arrays are
// registers, no scratch (K = 8: DESIGN.md 4.27 has the count).  MIX_BLOCKS blocks of MIX_THREADS lanes take contiguous
// ranges of row pairs, a lane its pairs lo + lane, lo + lane + MIX_THREADS, ... in order, first row before second.  The
// wide accesses need every array 16-byte aligned (VEC); otherwise the same lane takes the same two rows with 8- and
// 4-byte accesses, so no output bit depends on the alignment.  The last row of an odd B is a half pair.
//
// The loss sums follow inr_gain.hip's scheme, once per term: a lane's terms in row order, the fixed MIX_THREADS-lane tree
// of inr_reduce.h, ordered partials in loss_out[MIX_PARTIALS + term * MIX_BLOCKS + block], then one thread per term folds
// them in block order into loss_out[1 + term], and the total loss_out[0] is those K + 1 words added in order.  No
// atomics: the same inputs give the same bits on every call.
#include "inr_device.h"
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

namespace {

constexpr int MIX_THREADS = 512;  // 8 waves: two per SIMD, so a lane may hold up to 256 VGPRs (K = 8 needs more than 128)
constexpr int MIX_TERMS = MIX_MAX_HEADS + 1;
constexpr int MIX_APPLY_MAX_BLOCKS = 2048;
static_assert(MIX_PARTIALS + MIX_TERMS * MIX_BLOCKS <= 512, "the partials must fit INR_LOSS_WORDS");

template <int K>
__device__ __forceinline__ void mix_pre(const float (&w)[K], const float (&y)[K][2], bool clamp, float* pre, float* res) {
  // no contraction: res is the chain of rounded products and sums mix_numpy_f32 states, whether it comes from
  // inr_mix_loss_grad or inr_mix_apply
#pragma clang fp contract(off)
  float p0 = w[0] * y[0][0], p1 = w[0] * y[0][1];
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const float q0 = w[k] * y[k][0], q1 = w[k] * y[k][1];
    p0 = p0 + q0;
    p1 = p1 + q1;
  }
  pre[0] = p0, pre[1] = p1;
  res[0] = clamp ? fminf(fmaxf(p0, -1.f), 1.f) : p0;
  res[1] = clamp ? fminf(fmaxf(p1, -1.f), 1.f) : p1;
}

// one row: everything the kernel computes for it.  `live`: the row enters the loss.  acc[0] the mixed term, acc[1 + k]
// ring k's
template <int K>
__device__ __forceinline__ void mix_row(const LossDesc& ld, const MixArgs& a, bool live, float d, const float (&w)[K],
                                        const float (&y)[K][2], const float* t, float* res, float (&dy)[K][2],
                                        float (&dw)[K], float (&acc)[K + 1]) {
#pragma clang fp contract(off)
  float pre[2];
  mix_pre<K>(w, y, a.clamp != 0, pre, res);
#pragma unroll
  for (int k = 0; k < K; ++k) dy[k][0] = dy[k][1] = dw[k] = 0.f;
  if (!live) return;
  LossDesc l = ld;
  l.inv_count = a.inv_count[0];
  float dres[2] = {0.f, 0.f};
  acc[0] += loss_row(l, 2, res, t, dres);
  const float dp0 = (a.clamp == 0 || (pre[0] >= -1.f && pre[0] <= 1.f)) ? dres[0] : 0.f;
  const float dp1 = (a.clamp == 0 || (pre[1] >= -1.f && pre[1] <= 1.f)) ? dres[1] : 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float u0 = dp0 * y[k][0], u1 = dp1 * y[k][1];
    dw[k] = u0 + u1;
    float g[2] = {0.f, 0.f};
    if (a.radii[k] <= d && d <= a.radii[k + 1]) {
      l.inv_count = a.inv_count[1 + k];
      acc[1 + k] += loss_row(l, 2, y[k], t, g);
    }
    if (a.detach == 0) {
      const float v0 = w[k] * dp0, v1 = w[k] * dp1;
      g[0] = g[0] + v0;
      g[1] = g[1] + v1;
    }
    dy[k][0] = g[0], dy[k][1] = g[1];
  }
}

// the 2K floats of a lane's two rows of a row-major [B,K] array, from element r * K
template <int K, bool VEC>
__device__ __forceinline__ void load_rows(const float* __restrict__ p, long long r, bool two, float (&v)[2][K]) {
  const float* q = p + r * K;
  if (VEC && two) {
    float f[2 * K];
    if (K % 2 == 0) {
#pragma unroll
      for (int i = 0; i < K / 2; ++i) {
        const float4 x = reinterpret_cast<const float4*>(q)[i];
        f[4 * i] = x.x, f[4 * i + 1] = x.y, f[4 * i + 2] = x.z, f[4 * i + 3] = x.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float2 x = reinterpret_cast<const float2*>(q)[i];
        f[2 * i] = x.x, f[2 * i + 1] = x.y;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[0][k] = f[k], v[1][k] = f[K + k];
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      v[0][k] = q[k];
      v[1][k] = two ? q[K + k] : 0.f;
    }
  }
}

template <int K, bool VEC>
__device__ __forceinline__ void store_rows(float* __restrict__ p, long long r, bool two, const float (&v)[2][K]) {
  float* q = p + r * K;
  if (VEC && two) {
    float f[2 * K];
#pragma unroll
    for (int k = 0; k < K; ++k) f[k] = v[0][k], f[K + k] = v[1][k];
    if (K % 2 == 0) {
#pragma unroll
      for (int i = 0; i < K / 2; ++i)
        reinterpret_cast<float4*>(q)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < K; ++i) reinterpret_cast<float2*>(q)[i] = float2{f[2 * i], f[2 * i + 1]};
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      q[k] = v[0][k];
      if (two) q[K + k] = v[1][k];
    }
  }
}

// a lane's two rows of a [B,2] array: v[0..1] row r, v[2..3] row r + 1 (zeros when there is none)
template <bool VEC>
__device__ __forceinline__ void load_pair(const float* p, long long r, bool two, float* v) {
  if (VEC && two) {
    const float4 x = *reinterpret_cast<const float4*>(p + 2 * r);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
    const float2 x = reinterpret_cast<const float2*>(p)[r];
    const float2 z = two ? reinterpret_cast<const float2*>(p)[r + 1] : float2{0.f, 0.f};
    v[0] = x.x, v[1] = x.y, v[2] = z.x, v[3] = z.y;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_pair(float* p, long long r, bool two, const float* v) {
  if (VEC && two) {
    *reinterpret_cast<float4*>(p + 2 * r) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    reinterpret_cast<float2*>(p)[r] = float2{v[0], v[1]};
    if (two) reinterpret_cast<float2*>(p)[r + 1] = float2{v[2], v[3]};
  }
}

template <int K, bool VEC>
__global__ __launch_bounds__(MIX_THREADS) void mix_loss_grad_kernel(const LossDesc ld, const MixArgs a,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ gt,
                                                                    const float* __restrict__ dist,
                                                                    const uint8_t* __restrict__ mask, long long B,
                                                                    float* res, float* __restrict__ loss_out,
                                                                    float* __restrict__ dw) {
  __shared__ float red[MIX_THREADS];
  const long long pairs = (B + 1) >> 1;
  const long long per = (pairs + MIX_BLOCKS - 1) / MIX_BLOCKS;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < pairs ? lo + per : pairs;
  float acc[K + 1];
#pragma unroll
  for (int t = 0; t <= K; ++t) acc[t] = 0.f;
  for (long long p = lo + threadIdx.x; p < hi; p += MIX_THREADS) {
    const long long r = 2 * p;
    const bool two = r + 1 < B;  // false only for the last row of an odd B
    float wv[2][K], yv[2][K][2], tv[4], dv[2];
    load_rows<K, VEC>(w, r, two, wv);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float v[4];
      load_pair<VEC>(a.y[k], r, two, v);
      yv[0][k][0] = v[0], yv[0][k][1] = v[1], yv[1][k][0] = v[2], yv[1][k][1] = v[3];
    }
    load_pair<VEC>(gt, r, two, tv);
    if (VEC && two) {
      const float2 d2 = *reinterpret_cast<const float2*>(dist + r);
      dv[0] = d2.x, dv[1] = d2.y;
    } else {
      dv[0] = dist[r];
      dv[1] = two ? dist[r + 1] : 0.f;
    }
    float rv[4], dyv[2][K][2], dwv[2][K];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool have = j == 0 || two;
      const bool live = have && (mask == nullptr || mask[r + j] != 0);
      mix_row<K>(ld, a, live, dv[j], wv[j], yv[j], tv + 2 * j, rv + 2 * j, dyv[j], dwv[j], acc);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float v[4] = {dyv[0][k][0], dyv[0][k][1], dyv[1][k][0], dyv[1][k][1]};
      store_pair<VEC>(a.dy[k], r, two, v);
    }
    store_rows<K, VEC>(dw, r, two, dwv);
    if (res != nullptr) store_pair<VEC>(res, r, two, rv);
  }
#pragma unroll
  for (int t = 0; t <= K; ++t) {
    const float s = block_reduce<MIX_THREADS>(acc[t], red, Sum());
    if (threadIdx.x == 0) loss_out[MIX_PARTIALS + t * MIX_BLOCKS + blockIdx.x] = s;
  }
}

// loss_out[1 + t] = term t's partials in block order (thread t), then loss_out[0] = the terms in order (thread 0)
__global__ void mix_fold_kernel(int K, float* loss_out) {
  __shared__ float term[MIX_TERMS];
  const int t = threadIdx.x;
  if (t <= K) {
    float s = 0.f;
    for (int b = 0; b < MIX_BLOCKS; ++b) s += loss_out[MIX_PARTIALS + t * MIX_BLOCKS + b];
    term[t] = s;
    loss_out[1 + t] = s;
  }
  __syncthreads();
  if (t == 0) {
    float s = term[0];
    for (int k = 1; k <= K; ++k) s += term[k];
    loss_out[0] = s;
  }
}

// res alone: mix_pre, the function mix_row calls, so the bits equal inr_mix_loss_grad's res.  A lane reads its rows of
// every y_k before it writes res and touches no other lane's, so res == y[0] is allowed (no __restrict__ on them)
template <int K, bool VEC>
__global__ __launch_bounds__(256) void mix_apply_kernel(const MixArgs a, const float* __restrict__ w, long long B,
                                                        float* res) {
  const long long pairs = (B + 1) >> 1;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (long long)gridDim.x * 256) {
    const long long r = 2 * p;
    const bool two = r + 1 < B;
    float wv[2][K], yv[2][K][2], rv[4], pre[2];
    load_rows<K, VEC>(w, r, two, wv);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float v[4];
      load_pair<VEC>(a.y[k], r, two, v);
      yv[0][k][0] = v[0], yv[0][k][1] = v[1], yv[1][k][0] = v[2], yv[1][k][1] = v[3];
    }
    mix_pre<K>(wv[0], yv[0], a.clamp != 0, pre, rv);
    mix_pre<K>(wv[1], yv[1], a.clamp != 0, pre, rv + 2);
    store_pair<VEC>(res, r, two, rv);
  }
}

template <int K>
void mix_loss_grad_k(bool vec, const LossDesc& ld, const MixArgs& a, const float* w, const float* gt, const float* dist,
                     const uint8_t* mask, long long B, float* res, float* loss_out, float* dw, hipStream_t st) {
  auto* k = vec ? mix_loss_grad_kernel<K, true> : mix_loss_grad_kernel<K, false>;
  hipLaunchKernelGGL(k, dim3(MIX_BLOCKS), dim3(MIX_THREADS), 0, st, ld, a, w, gt, dist, mask, B, res, loss_out, dw);
}

template <int K>
void mix_apply_k(bool vec, unsigned blocks, const MixArgs& a, const float* w, long long B, float* res, hipStream_t st) {
  auto* k = vec ? mix_apply_kernel<K, true> : mix_apply_kernel<K, false>;
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, st, a, w, B, res);
}

bool mix_tables_aligned(const MixArgs& a, bool with_dy) {
  uintptr_t bits = 0;
  for (int k = 0; k < a.n_heads; ++k) bits |= (uintptr_t)a.y[k] | (with_dy ? (uintptr_t)a.dy[k] : 0);
  return (bits & 15u) == 0;
}

}  // namespace

hipError_t launch_mix_loss_grad(const LossDesc& ld, const MixArgs& a, const float* w, const float* gt, const float* dist,
                                const uint8_t* mask, long long B, float* res, float* loss_out, float* dw, hipStream_t st) {
  const bool vec = mix_tables_aligned(a, true) &&
                   (((uintptr_t)w | (uintptr_t)dw | (uintptr_t)gt | (uintptr_t)res) & 15u) == 0 && ((uintptr_t)dist & 7u) == 0;
  switch (a.n_heads) {
    case 2: mix_loss_grad_k<2>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    case 3: mix_loss_grad_k<3>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    case 4: mix_loss_grad_k<4>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    case 5: mix_loss_grad_k<5>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    case 6: mix_loss_grad_k<6>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    case 7: mix_loss_grad_k<7>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    case 8: mix_loss_grad_k<8>(vec, ld, a, w, gt, dist, mask, B, res, loss_out, dw, st); break;
    default: return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(mix_fold_kernel, dim3(1), dim3(16), 0, st, a.n_heads, loss_out);
  return hipGetLastError();
}

hipError_t launch_mix_apply(const MixArgs& a, const float* w, long long B, float* res, hipStream_t st) {
  const long long pairs = (B + 1) >> 1;
  const long long want = (pairs + 255) / 256;
  const unsigned blocks = (unsigned)(want < MIX_APPLY_MAX_BLOCKS ? want : MIX_APPLY_MAX_BLOCKS);
  const bool vec = mix_tables_aligned(a, false) && (((uintptr_t)w | (uintptr_t)res) & 15u) == 0;
  switch (a.n_heads) {
    case 2: mix_apply_k<2>(vec, blocks, a, w, B, res, st); break;
    case 3: mix_apply_k<3>(vec, blocks, a, w, B, res, st); break;
    case 4: mix_apply_k<4>(vec, blocks, a, w, B, res, st); break;
    case 5: mix_apply_k<5>(vec, blocks, a, w, B, res, st); break;
    case 6: mix_apply_k<6>(vec, blocks, a, w, B, res, st); break;
    case 7: mix_apply_k<7>(vec, blocks, a, w, B, res, st); break;
    case 8: mix_apply_k<8>(vec, blocks, a, w, B, res, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace inr
