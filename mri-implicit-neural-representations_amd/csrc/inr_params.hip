// inr_params.hip -- the tail of every training step (gfx950): slab reduction, Adam fused with the re-pack of the weight
// images, penalty gradients.  Coalesced streaming kernels, HBM-bound; every sum runs in a fixed order.
#include <algorithm>
#include <cstdlib>
#include "inr_device.h"
#include "inr_aux.h"
#include "inr_w2.h"
#include "inr_reduce.h"

namespace inr {

// ---------------------------------------------------------------------------------------------
// Flat-parameter element -> where it lives in the virtual real matrices the fused kernel works on.
// A flat float is a real weight (LT_REAL, LT_WIRE_FIRST), the Re or Im part of a complex weight
// (LT_WIRE_HIDDEN: W = Wr + jWi acts as [[Wr,-Wi],[Wi,Wr]] on interleaved (Re,Im) rows;
// LT_WIRE_LAST: only the real output row [Wr,-Wi] exists), or a bias entry.
// ---------------------------------------------------------------------------------------------
struct VirtualPos {
  int n;          // number of virtual entries (0, 1 or 2)
  int row[2], col[2];
  float sign[2];
  int bias_row;   // >= 0: this flat element is a bias entry of that virtual row (n == 0)
};

__device__ __forceinline__ bool locate(const NetDesc& nd, int i, int& l, VirtualPos& vp) {
  vp.n = 0;
  vp.bias_row = -1;
  for (l = 0; l < nd.ND; ++l) {
    const LayerDesc& L = nd.L[l];
    const int off = i - L.w_off;
    if (off >= 0 && off < L.wn) {
      if (L.ltype == LT_REAL || L.ltype == LT_GABOR_MU) {
        vp.n = 1; vp.row[0] = off / L.K; vp.col[0] = off - vp.row[0] * L.K; vp.sign[0] = 1.f;
      } else if (L.ltype == LT_WIRE_FIRST) {
        const int r = off / L.K;
        vp.n = 1; vp.row[0] = 2 * r; vp.col[0] = off - r * L.K; vp.sign[0] = 1.f;
      } else {
        const int kc = L.K >> 1;  // complex in-features
        const int r = off / (2 * kc), rem = off - r * 2 * kc, j = rem >> 1, c = rem & 1;
        if (L.ltype == LT_WIRE_HIDDEN) {
          vp.n = 2;
          if (c == 0) {  // Wr -> (2r,2j) and (2r+1,2j+1)
            vp.row[0] = 2 * r; vp.col[0] = 2 * j; vp.sign[0] = 1.f;
            vp.row[1] = 2 * r + 1; vp.col[1] = 2 * j + 1; vp.sign[1] = 1.f;
          } else {       // Wi -> +(2r+1,2j) and -(2r,2j+1)
            vp.row[0] = 2 * r + 1; vp.col[0] = 2 * j; vp.sign[0] = 1.f;
            vp.row[1] = 2 * r; vp.col[1] = 2 * j + 1; vp.sign[1] = -1.f;
          }
        } else {  // LT_WIRE_LAST: out = Re(W h + beta): row r = [Wr, -Wi]
          vp.n = 1; vp.row[0] = r; vp.col[0] = 2 * j + c; vp.sign[0] = c ? -1.f : 1.f;
        }
      }
      return true;
    }
    const int ob = i - L.b_off;
    if (ob >= 0 && ob < L.bn) {
      if (L.ltype == LT_REAL || L.ltype == LT_GABOR_MU) vp.bias_row = ob;
      else if (L.ltype == LT_WIRE_FIRST) vp.bias_row = 2 * ob;
      else if (L.ltype == LT_WIRE_HIDDEN) vp.bias_row = ob;            // (i, c) -> row 2i + c
      else vp.bias_row = (ob & 1) ? -2 : (ob >> 1);                    // imaginary output bias: no effect
      return true;
    }
  }
  return false;
}

// Sum of the per-slab loss words by one whole workgroup (the extra last one of the reduction grids): lane t adds
// slabs t, t + 256, ..., then a fixed LDS tree -- reproducible, and 196 dependent cache misses shorter than the
// single-thread loop it replaces (which was the critical path of the whole reduction kernel).
__device__ __forceinline__ void loss_words_sum(const float* __restrict__ slabs, int n, size_t stride, int off,
                                               float* __restrict__ loss_out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int b = threadIdx.x; b < n; b += 256) s += slabs[(size_t)b * stride + off];
  s = block_reduce_once<256>(s, red, Sum());
  if (threadIdx.x == 0) loss_out[0] = s;
}

// ---------------------------------------------------------------------------------------------
// grads[i] = sum over blocks (in block order: deterministic) of the slab entries that flat
// element i owns; the loss words are summed by the grid's extra last workgroup (loss_words_sum).
// ---------------------------------------------------------------------------------------------
// sum of n slab entries `stride` floats apart, 16 independent loads in flight, added in slab order
__device__ __forceinline__ float slab_sum(const float* __restrict__ p, size_t stride, int n) {
  float s = 0.f;
  int b = 0;
  for (; b + 16 <= n; b += 16) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = p[(size_t)(b + k) * stride];
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
  }
  // the tail the same way (clamped addresses, selects after the loads): a chunk-slab set of 23 is a batch of 16 and then 7
  // -- as a scalar loop those were 7 serialized L2 / HBM round trips.  A short tail takes a short batch (wave-uniform n): the
  // 4 chunk slabs of the 8 x 512 filter network were 16 loads per entry, 12 of them of the same word.
  if (n - b > 4) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = p[(size_t)(b + k < n ? b + k : n - 1) * stride];
#pragma unroll
    for (int k = 0; k < 16; ++k) s += b + k < n ? v[k] : 0.f;
  } else if (b < n) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[(size_t)(b + k < n ? b + k : n - 1) * stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) s += b + k < n ? v[k] : 0.f;
  }
  return s;
}

__global__ __launch_bounds__(256) void reduce_slabs_kernel(const NetDesc nd, const float* __restrict__ slabs_all,
                                                           int n_blocks_all, float* __restrict__ grads,
                                                           float* __restrict__ loss_out, SlabSplit split) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t sf = (size_t)nd.slab_floats;
  if (i < nd.P) {
    int l;
    VirtualPos vp;
    float s = 0.f;
    if (locate(nd, i, l, vp) && nd.L[l].live != 0) {  // dead layers: slab region never written -> 0
      const LayerDesc& L = nd.L[l];
      const bool second = split.n2 > 0 && ((((split.mask >> l) & 1u) != 0) || (i >= split.lo && i < split.hi));
      const float* __restrict__ slabs = second ? slabs_all + (size_t)n_blocks_all * sf : slabs_all;
      const int n_blocks = second ? split.n2 : n_blocks_all;
      if (vp.n >= 1) {
        const size_t o0 = (size_t)L.gw_off + (size_t)vp.row[0] * L.K + vp.col[0];
        s = vp.sign[0] * slab_sum(slabs + o0, sf, n_blocks);
        if (vp.n == 2) {
          const size_t o1 = (size_t)L.gw_off + (size_t)vp.row[1] * L.K + vp.col[1];
          s += vp.sign[1] * slab_sum(slabs + o1, sf, n_blocks);
        }
      } else if (vp.bias_row >= 0) {
        s = slab_sum(slabs + (size_t)L.gb_off + vp.bias_row, sf, n_blocks);
      }
    }
    grads[i] = s;
  }
  if (loss_out != nullptr && blockIdx.x == gridDim.x - 1) loss_words_sum(slabs_all, n_blocks_all, sf, nd.slab_loss_off, loss_out);
}

// Fast path when a slab has the flat-parameter layout (every layer LT_REAL).  A workgroup owns 256
// consecutive gradient entries (64 lanes x 16 B); its four waves each sum a contiguous quarter of
// the slabs (8 independent 16-byte loads in flight per lane) and the quarters are combined through
// LDS in wave order -- a fixed summation tree, so results are bitwise reproducible.  Returns, in every
// wave, the sum of the lane's entries i4 .. i4 + 3 (i4 = 4 * (64 * block + lane)); `part` is the caller's.
// split.lo / split.hi (lo3 / hi3) are multiples of 4 (slabs_flat): a lane's four entries share a slab set.
__device__ __forceinline__ f32x4 flat_slab_sum(const float* __restrict__ slabs_all, int n_blocks_all, int slab_floats,
                                               int P, const SlabSplit& split, f32x4 (*part)[64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i4 = (blockIdx.x * 64 + lane) * 4;
  const bool second = split.n2 > 0 && i4 >= split.lo && i4 < split.hi;
  const float* __restrict__ slabs = second ? slabs_all + (size_t)n_blocks_all * slab_floats : slabs_all;
  const int n_blocks = second ? (split.n3 > 0 && i4 >= split.lo3 && i4 < split.hi3 ? split.n3 : split.n2) : n_blocks_all;
  const int per = (n_blocks + 3) / 4;
  const int b0 = w * per, b1 = (b0 + per < n_blocks) ? b0 + per : n_blocks;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i4 < P) {
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(slabs + (size_t)(b + u) * slab_floats + i4);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < b1; ++b) s += *reinterpret_cast<const f32x4*>(slabs + (size_t)b * slab_floats + i4);
  }
  part[w][lane] = s;
  __syncthreads();
  return ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// the flat-layout reduction: flat_slab_sum, wave 0 stores the lane's four entries
__global__ __launch_bounds__(256) void reduce_slabs_real_kernel(const float* __restrict__ slabs_all, int n_blocks_all,
                                                                int slab_floats, int P, int loss_off,
                                                                float* __restrict__ grads,
                                                                float* __restrict__ loss_out, SlabSplit split) {
  __shared__ f32x4 part[4][64];
  const int i4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const f32x4 t = flat_slab_sum(slabs_all, n_blocks_all, slab_floats, P, split, part);
  if (threadIdx.x < 64 && i4 < P)
    for (int j = 0; j < 4 && i4 + j < P; ++j) grads[i4 + j] = t[j];
  if (loss_out != nullptr && blockIdx.x == gridDim.x - 1) loss_words_sum(slabs_all, n_blocks_all, (size_t)slab_floats, loss_off, loss_out);
}

// GaborLayer centres (mfn.py:116-131).  The fused kernel leaves, per filter and row j,
//   S1[j,k] = sum_c a_cj x_ck,  s0_j = sum_c a_cj,  T_j = sum_c a_cj |x_c|^2      (a = g_h * h, so that
// d h / d q = h * gamma with q = mu_j . x, and D = |x|^2 + |mu_j|^2 - 2 q); after the block reduction
// grads[mu] holds S1 and grads[gamma] holds s0.  This kernel (one wave per row) finishes
//   d gamma_j = -0.5 (T_j + |mu_j|^2 s0_j - 2 sum_k mu_jk S1_jk),   d mu_jk = gamma_j (S1_jk - s0_j mu_jk).
__global__ __launch_bounds__(64) void gabor_finish_kernel(const NetDesc nd, const float* __restrict__ slabs,
                                                          int n_blocks, const float* __restrict__ params,
                                                          const float* __restrict__ packed, float* __restrict__ grads) {
  const LayerDesc& L = nd.L[nd.mu0 + blockIdx.y];
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= L.M) return;
  const int NBW = nd.NB * 32;
  float t = 0.f, dot = 0.f;
  for (int b = lane; b < n_blocks; b += 64) t += slabs[(size_t)b * nd.slab_floats + L.gb_off + NBW + j];
  const float* mu = params + L.w_off + (size_t)j * L.K;
  float* g = grads + L.w_off + (size_t)j * L.K;
  for (int k = lane; k < L.K; k += 64) dot = fmaf(mu[k], g[k], dot);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    t += __shfl_xor(t, off);
    dot += __shfl_xor(dot, off);
  }
  const float s0 = grads[L.b_off + j], gamma = params[L.b_off + j], m2 = packed[L.pbias_off + NBW + j];
  for (int k = lane; k < L.K; k += 64) g[k] = gamma * (g[k] - s0 * mu[k]);
  if (lane == 0) grads[L.b_off + j] = -0.5f * ((t + m2 * s0) - 2.f * dot);
}

// |mu_j|^2 into the second half of the centre layer's bias image (after every (re)pack of the parameters)
__global__ __launch_bounds__(64) void gabor_m2_kernel(const NetDesc nd, const float* __restrict__ params,
                                                      float* __restrict__ packed) {
  const LayerDesc& L = nd.L[nd.mu0 + blockIdx.y];
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= L.M) return;
  const float* mu = params + L.w_off + (size_t)j * L.K;
  float s = 0.f;
  for (int k = lane; k < L.K; k += 64) s = fmaf(mu[k], mu[k], s);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) packed[L.pbias_off + nd.NB * 32 + j] = s;
}

// every layer is LT_REAL (with_mu: or a Gabor centre layer, whose entries are real too)
static bool layers_real(const NetDesc& nd, bool with_mu) {
  for (int l = 0; l < nd.ND; ++l)
    if (nd.L[l].ltype != LT_REAL && !(with_mu && nd.L[l].ltype == LT_GABOR_MU)) return false;
  return true;
}

// slab layout == flat layout for this split: real layers at their flat offsets (not the case for MFN: L[] order != flat
// order; slab_floats % 64 == 0 keeps every slab 16-byte aligned), no per-layer slab set, and the bounds of the slab sets
// in use at multiples of 4 (a lane's four entries share a slab set)
static bool slabs_flat(const NetDesc& nd, const SlabSplit& split) {
  for (int l = 0; l < nd.ND; ++l)
    if (nd.L[l].gw_off != nd.L[l].w_off) return false;
  return layers_real(nd, false) && split.mask == 0 && ((split.lo | split.hi) & 3) == 0 &&
         (split.n3 == 0 || ((split.lo3 | split.hi3) & 3) == 0);
}

// the layers lie in the flat vector in L[] order, weights then bias, without gaps (AdamArgs::flat_order; not the filter
// networks: state_dict order != L[] order)
static bool layers_flat_order(const NetDesc& nd) {
  int off = 0;
  for (int l = 0; l < nd.ND; ++l) {
    if (nd.L[l].w_off != off || nd.L[l].b_off != off + nd.L[l].wn) return false;
    off += nd.L[l].wn + nd.L[l].bn;
  }
  return off == nd.P;
}

hipError_t launch_reduce_slabs(const NetDesc& nd, const float* slabs, int n_blocks, float* grads, float* loss_out,
                               const float* params, const float* packed, hipStream_t st, SlabSplit split) {
  const bool flat = slabs_flat(nd, split);
  if (split.n3 > 0 && !flat) return hipErrorInvalidValue;  // a third slab count is the flat-layout reduction's only
  const int grid = (nd.P + 255) / 256;
  if (flat)
    hipLaunchKernelGGL(reduce_slabs_real_kernel, dim3(grid + 1), dim3(256), 0, st, slabs, n_blocks, nd.slab_floats, nd.P,
                       nd.slab_loss_off, grads, loss_out, split);
  else
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(grid + 1), dim3(256), 0, st, nd, slabs, n_blocks, grads, loss_out, split);
  if (nd.gabor)
    hipLaunchKernelGGL(gabor_finish_kernel, dim3(nd.L[nd.mu0].M, nd.mfn_n + 1), dim3(64), 0, st, nd, slabs, n_blocks,
                       params, packed, grads);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam single-tensor algorithm, amsgrad=False; train.py:76,190) fused with the
// re-pack of every weight into the two MFMA A-fragment images and of every bias into its padded
// bias image.  do_update == 0: pack only.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_fwd(const NetDesc& nd, const LayerDesc& L, int l, float* packed, int row, int k,
                                        float v) {
  int h, s;
  if (L.korder == 1) {
    h = k >= nd.E;
    s = h ? k - nd.E : k;
  } else {
    h = k & 1;
    s = k >> 1;
  }
  packed[L.pf_off + ((size_t)((s >> 2) * L.Mblk + (row >> 5)) * 64 + h * 32 + (row & 31)) * 4 + (s & 3)] = v;
}

__device__ __forceinline__ void put_tr(const LayerDesc& L, float* packed, int row, int k, float v) {
  const int h = row & 1, s = row >> 1;  // transposed image A'[i=k][k'=row]
  packed[L.pb_off + ((size_t)((s >> 2) * L.Kblk + (k >> 5)) * 64 + h * 32 + (k & 31)) * 4 + (s & 3)] = v;
}

// Fragment images of the row-split fused step (inr_mlp_rs_impl.h): v_mfma_f32_16x16x4_f32 A operands, one float4 per lane
// and k-step = the four 16-row blocks of a wave's 64 rows: W[row][k] -> float4 ((k >> 2) * 4 + (row >> 6)) * 64 +
// (k & 3) * 16 + (row & 15), component (row >> 4) & 3.  Layer 0 keeps its k in CHUNK order: 32 encoder phases at a time,
// their sines then their cosines (the kernel generates the features chunk by chunk).
__device__ __forceinline__ void put_rs(const NetDesc& nd, const LayerDesc& L, int l, float* packed, int row, int k, float v) {
  if (l >= nd.D - 1) return;  // the last layer's rows are read from the flat parameters
  int kk = k;
  if (l == 0) {
    const int trig = k >= nd.E, sp = trig ? k - nd.E : k;
    kk = (sp >> 5) * 64 + trig * 32 + (sp & 31);
  }
  packed[L.rf_off + ((size_t)(((kk >> 2) * 4 + (row >> 6)) * 64 + (kk & 3) * 16 + (row & 15))) * 4 + ((row >> 4) & 3)] = v;
  if (l >= 1)  // transposed image A'[i = k][k' = row]
    packed[L.rb_off + ((size_t)(((row >> 2) * 4 + (k >> 6)) * 64 + (row & 3) * 16 + (k & 15))) * 4 + ((k >> 4) & 3)] = v;
}

// "Weight panels in LDS" images of the bf16 path (inr_siren_bf16_impl.h; layout and the constant factors that ride in the
// images: inr_w2.h): weight W_l[row][k] goes into the forward panels of layer l -- times w0 / 2 pi for the sine layers, so
// that their accumulators are phases in revolutions -- and, for l >= 1, into the transposed panels (out index = k,
// contraction index = row) times the w0 of the layer below; biases into the fp32 table, scaled like their weights.
// Plain SIREN plans only (every layer LT_REAL, hidden rows = 256 padded).
__device__ __forceinline__ float w2_krev(const NetDesc& nd, int l) {
  return l < nd.D - 1 ? nd.L[l].omega * 0.15915494309189535f : 1.0f;
}
__device__ __forceinline__ void put_w2(const NetDesc& nd, int l, float* packed, int row, int k, float v) {
  __bf16* img = reinterpret_cast<__bf16*>(packed + nd.w2_off);
  const int D = nd.D, E = nd.E;
  int t, h, j;
  if (l == 0) {  // gauss features: K-step t holds frequencies 8t .. 8t+7 -- lane half h the four 8t + 4h .. + 3, as (sine,
    // cosine) pairs in elements (2i, 2i+1): one phase chain per pair in the kernel; two K-steps per panel
    const int trig = k >= E;
    const int kk = trig ? k - E : k;
    t = kk >> 3;
    h = (kk & 7) >> 2;
    j = 2 * (kk & 3) + trig;
    img[w2_index(t >> 1, (t & 1) * 8 + (row >> 5), h * 32 + (row & 31), j)] = (__bf16)(v * w2_krev(nd, 0));
  } else {
    w2_kperm_inv(k, t, h, j);
    if (l == D - 1)  // last layer (rows < 32): one panel, its 16 K-steps
      img[w2_index(w2_p_last(D, E), t, h * 32 + row, j)] = (__bf16)v;
    else
      img[w2_index(w2_p_fwd(l, E) + (row >> 5), t, h * 32 + (row & 31), j)] = (__bf16)(v * w2_krev(nd, l));
    w2_kperm_inv(row, t, h, j);
    const float vt = v * nd.L[l - 1].omega;
    if (l == D - 1)  // one K-step (rows < 4: t = 0), eight row blocks
      img[w2_index(w2_p_lastT(D, E), k >> 5, h * 32 + (k & 31), j)] = (__bf16)vt;
    else
      img[w2_index(w2_p_T(l, D, E) + (k >> 5), t, h * 32 + (k & 31), j)] = (__bf16)vt;
  }
}

// one flat entry: the Adam update from gradient `g` (do_update); returns the entry's (new) value.  `p`, `m`, `v`: the
// entry's parameter and moments as loaded by the caller (the fused kernel loads them before the slab reduction: their
// latency hides behind the slab loads instead of following them)
__device__ __forceinline__ float adam_update_loaded(const NetDesc& nd, int i, float g, float p, float m, float v,
                                                    float* __restrict__ params, float* __restrict__ m1,
                                                    float* __restrict__ m2, const AdamArgs& aa) {
  bool live = true;
  if (aa.has_dead) {
    if (aa.n_dead >= 0) {  // (a handful of ranges in kernel arguments: scalar compares -- the walk over 26 layer descriptors
      for (int r = 0; r < aa.n_dead; ++r)  //  below was most of the update's time on the 8 x 512 filter network)
        if (i >= aa.dead_lo[r] && i < aa.dead_hi[r]) live = false;
    } else {
      for (int l = 0; l < nd.ND; ++l) {
        const LayerDesc& L = nd.L[l];
        if ((i >= L.w_off && i < L.w_off + L.wn) || (i >= L.b_off && i < L.b_off + L.bn)) live = L.live != 0;
      }
    }
  }
  if (aa.do_update && live) {
    if (aa.weight_decay != 0.f) g = fmaf(aa.weight_decay, p, g);
    if (aa.l1 != 0.f) g += aa.l1 * (p > 0.f ? 1.f : (p < 0.f ? -1.f : 0.f));  // d/dp lambda*sum|p|
    if (aa.l2 != 0.f) g = fmaf(2.f * aa.l2, p, g);                             // d/dp lambda*|sum p^2|
    float step_size = aa.step_size, bc2_sqrt = aa.bc2_sqrt;
    if (aa.sched != nullptr) {  // wave-uniform: scalar loads
      const int t = min(*aa.step_dev, aa.n_sched - 1);
      step_size = aa.sched[2 * t];
      bc2_sqrt = aa.sched[2 * t + 1];
    }
    m = m + (g - m) * aa.omb1;                // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(g * g, aa.omb2, v * aa.beta2);   // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + aa.eps;
    p = p - step_size * (m / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
    m1[i] = m;
    m2[i] = v;
    params[i] = p;
  }
  return p;
}

__device__ __forceinline__ float adam_update_entry(const NetDesc& nd, int i, float g, float* __restrict__ params,
                                                   float* __restrict__ m1, float* __restrict__ m2, const AdamArgs& aa) {
  const bool upd = aa.do_update != 0;  // (pack only: there are no moments)
  return adam_update_loaded(nd, i, g, params[i], upd ? m1[i] : 0.f, upd ? m2[i] : 0.f, params, m1, m2, aa);
}

// Where a workgroup's 256 consecutive flat entries start looking for their layer: with the layers in flat order (AdamArgs::
// flat_order: weights then bias, layer after layer) the walk begins at the first layer that ends behind the workgroup's
// first entry and stops with the one that holds its last -- one or two layers, found once per workgroup with scalar
// loads, where every entry used to walk the list from the top.  Otherwise: the whole list.
struct LayerWalk {
  int l0, i_last;
};
__device__ __forceinline__ LayerWalk layer_walk(const NetDesc& nd, const AdamArgs& aa, int first) {
  LayerWalk lw = {0, 0x7fffffff};
  if (aa.flat_order) {
    while (lw.l0 < nd.ND - 1 && nd.L[lw.l0].b_off + nd.L[lw.l0].bn <= first) ++lw.l0;
    lw.i_last = first + 255;
  }
  return lw;
}

// the image entries of flat entry i, value p -- those of the sets aa.skip_sets leaves out stay as they are (the host marks
// them stale: inr_host.h)
__device__ __forceinline__ void pack_entry(const NetDesc& nd, int i, float p, float* __restrict__ packed, const AdamArgs& aa,
                                           const LayerWalk& lw) {
  const int skip = aa.skip_sets;
  if (aa.all_real) {  // SIREN / FFN: one weight entry or one bias entry, no sign, no pair
    for (int l = lw.l0; l < nd.ND; ++l) {  // (l is wave-uniform: the descriptors stay scalar loads)
      const LayerDesc& L = nd.L[l];
      const int off = i - L.w_off;
      if (off >= 0 && off < L.wn) {
        // K a power of two (every hidden layer of the built widths 32 .. 512, every gauss encoder of 2^n phases): a shift
        const int row = (L.K & (L.K - 1)) == 0 ? off >> (31 - __clz(L.K)) : off / L.K, k = off - row * L.K;
        if (nd.bf16) {  // bf16 plans keep the panel stream only
          put_w2(nd, l, packed, row, k, p);
          return;
        }
        if (!(skip & IMG_FWD)) put_fwd(nd, L, l, packed, row, k, p);
        if (!(skip & IMG_TR) && L.pb_off >= 0) put_tr(L, packed, row, k, p);
        if (!(skip & IMG_RS) && nd.rs) put_rs(nd, L, l, packed, row, k, p);
        return;
      }
      const int ob = i - L.b_off;
      if (ob >= 0 && ob < L.bn) {
        if (nd.bf16)
          packed[nd.w2_bias_off + l * 256 + ob] = p * w2_krev(nd, l);
        else
          packed[L.pbias_off + ob] = p;
        return;
      }
      if (L.b_off + L.bn > lw.i_last) return;  // (flat order: nothing of this workgroup lies behind this layer)
    }
    return;
  }
  int l;
  VirtualPos vp;
  if (!locate(nd, i, l, vp)) return;
  const LayerDesc& L = nd.L[l];
  for (int t = 0; t < vp.n; ++t) {
    put_fwd(nd, L, l, packed, vp.row[t], vp.col[t], vp.sign[t] * p);
    if (L.pb_off >= 0) put_tr(L, packed, vp.row[t], vp.col[t], vp.sign[t] * p);
  }
  if (vp.bias_row >= 0) packed[L.pbias_off + vp.bias_row] = p;
}

// one flat entry: Adam update (adam_update_entry), then its image entries
__device__ __forceinline__ void adam_pack_entry(const NetDesc& nd, int i, float g, float* __restrict__ params,
                                                float* __restrict__ m1, float* __restrict__ m2,
                                                float* __restrict__ packed, const AdamArgs& aa, const LayerWalk& lw) {
  pack_entry(nd, i, adam_update_entry(nd, i, g, params, m1, m2, aa), packed, aa, lw);
}

__global__ __launch_bounds__(256) void adam_pack_kernel(const NetDesc nd, float* __restrict__ params,
                                                        const float* __restrict__ grads, float* __restrict__ m1,
                                                        float* __restrict__ m2, float* __restrict__ packed,
                                                        AdamArgs aa) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const LayerWalk lw = layer_walk(nd, aa, blockIdx.x * 256);
  if (i >= nd.P) return;
  adam_pack_entry(nd, i, aa.do_update ? grads[i] : 0.f, params, m1, m2, packed, aa, lw);
}

// reduce_slabs_real_kernel + adam_pack_kernel in one launch (single-rank steps: nothing sits between the reduction and
// the update).  Same summation (flat_slab_sum), same update arithmetic: bit-identical to the two launches; the gradient
// is still written (callers read it).  After the reduction wave 0 leaves the lanes' sums in LDS as 256 consecutive floats
// and thread t takes flat entry 256 * block + t: gradient, parameter and both moments are one coalesced 4-byte access per
// thread and array (each wave used to take every fourth entry: all four waves touched every cache line of all three).
__global__ __launch_bounds__(256) void reduce_adam_real_kernel(const NetDesc nd, const float* __restrict__ slabs_all,
                                                               int n_blocks_all, float* __restrict__ grads,
                                                               float* __restrict__ loss_out, SlabSplit split,
                                                               float* __restrict__ params, float* __restrict__ m1,
                                                               float* __restrict__ m2, float* __restrict__ packed,
                                                               AdamArgs aa) {
  __shared__ f32x4 part[4][64];
  __shared__ f32x4 sum4[64];
  const int P = nd.P, i = blockIdx.x * 256 + threadIdx.x;
  float p = 0.f, m = 0.f, v = 0.f;
  if (i < P) p = params[i], m = m1[i], v = m2[i];  // (in flight beside the slab loads)
  const f32x4 t = flat_slab_sum(slabs_all, n_blocks_all, nd.slab_floats, P, split, part);
  if (threadIdx.x < 64) sum4[threadIdx.x] = t;
  const LayerWalk lw = layer_walk(nd, aa, blockIdx.x * 256);
  __syncthreads();
  if (i < P) {
    const float g = reinterpret_cast<const float*>(sum4)[threadIdx.x];
    grads[i] = g;
    pack_entry(nd, i, adam_update_loaded(nd, i, g, p, m, v, params, m1, m2, aa), packed, aa, lw);
  }
  if (loss_out != nullptr && blockIdx.x == gridDim.x - 1)
    loss_words_sum(slabs_all, n_blocks_all, (size_t)nd.slab_floats, nd.slab_loss_off, loss_out);
}

// Sharded data-parallel update: the entries [lo, hi) of the flat vector, gradient = this rank's chunk of the
// reduce-scatter (grads_shard[i - lo]); no image is written -- every rank re-packs after the all-gather of the parameters.
__global__ __launch_bounds__(256) void adam_shard_kernel(const NetDesc nd, float* __restrict__ params,
                                                         const float* __restrict__ grads_shard, float* __restrict__ m1,
                                                         float* __restrict__ m2, int lo, int hi, AdamArgs aa) {
  const int i = lo + blockIdx.x * 256 + threadIdx.x;
  if (i >= hi) return;
  adam_update_entry(nd, i, grads_shard[i - lo], params, m1, m2, aa);
}

// The images of LT_REAL layers written in IMAGE order (one float4 slot per thread, blockIdx.y = layer): coalesced
// stores, the weights gathered through the L2 -- where adam_pack_entry scatters 4-byte stores (16 segments per wave).
// Slots: forward image Kpad8 * Mblk * 8 | transposed image Mpad8 * Kblk * 8 (if any) | bias image Mblk * 8; padding slots
// are written as zeros (what they hold anyway).  The inverse of put_fwd / put_tr above.
__global__ __launch_bounds__(256) void pack_images_real_kernel(const NetDesc nd, const float* __restrict__ params,
                                                               float* __restrict__ packed) {
  const LayerDesc& L = nd.L[blockIdx.y];
  const int nf = L.Kpad8 * L.Mblk * 8, nt = L.pb_off >= 0 ? L.Mpad8 * L.Kblk * 8 : 0, nb = L.Mblk * 8;
  int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nf + nt + nb) return;
  const float* __restrict__ W = params + L.w_off;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (q < nf) {
    const int lane = q & 63, g = (q >> 6) / L.Mblk, mb = (q >> 6) - g * L.Mblk;
    const int h = lane >> 5, row = mb * 32 + (lane & 31);
    if (row < L.M) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int sidx = 4 * g + c;
        const int k = L.korder == 1 ? (sidx < nd.E ? h * nd.E + sidx : L.K) : 2 * sidx + h;
        if (k < L.K) v[c] = W[(size_t)row * L.K + k];
      }
    }
    *reinterpret_cast<f32x4*>(packed + L.pf_off + (size_t)q * 4) = v;
    return;
  }
  q -= nf;
  if (q < nt) {
    const int lane = q & 63, g = (q >> 6) / L.Kblk, kb = (q >> 6) - g * L.Kblk;
    const int h = lane >> 5, k = kb * 32 + (lane & 31);
    if (k < L.K) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int row = 2 * (4 * g + c) + h;
        if (row < L.M) v[c] = W[(size_t)row * L.K + k];
      }
    }
    *reinterpret_cast<f32x4*>(packed + L.pb_off + (size_t)q * 4) = v;
    return;
  }
  q -= nt;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (4 * q + c < L.bn) v[c] = params[L.b_off + 4 * q + c];
  *reinterpret_cast<f32x4*>(packed + L.pbias_off + (size_t)q * 4) = v;
}

// Gradient of the penalties of models/regularization.py:21-36 added to the flat gradient entries [lo, hi) (grads[i - lo]),
// for plans with complex64 tensors too (WIRE / WIRE2D hidden and last layers, stored as interleaved (re, im) pairs):
//   L1  lambda * sum |p|:  real entries sign(p); a complex z = a + ib contributes |z|, i.e. (a, b) / |z| (0 at z = 0)
//   L2  lambda * |S|, S = sum p^2 over every Parameter -- a COMPLEX sum when the model has complex tensors (z^2 = a^2 - b^2
//       + 2iab):  with u = conj(S) / |S| = (ur, ui):  real entry 2 p ur;  d/da = 2 (ur a - ui b),  d/db = -2 (ur b + ui a).
// u is read from device memory (the caller forms S, which also holds the squares of the frozen omega_0 / scale_0
// Parameters, networks.py:191-192); l2_dir == nullptr means u = (1, 0): all-real models.  Reads params, writes grads only:
// a pair's two entries never race.
__global__ __launch_bounds__(256) void reg_grad_kernel(const NetDesc nd, const float* __restrict__ params,
                                                       float* __restrict__ grads, int lo, int hi, float l1, float l2,
                                                       const float* __restrict__ l2_dir) {
  const int i = lo + blockIdx.x * 256 + threadIdx.x;
  if (i >= hi) return;
  int role = 0;  // 0: real entry, 1 / 2: real / imaginary part of a complex entry
  for (int l = 0; l < nd.ND; ++l) {
    const LayerDesc& L = nd.L[l];
    if (L.ltype != LT_WIRE_HIDDEN && L.ltype != LT_WIRE_LAST) continue;
    const int off = i - L.w_off, ob = i - L.b_off;
    if (off >= 0 && off < L.wn) role = 1 + (off & 1);
    if (ob >= 0 && ob < L.bn) role = 1 + (ob & 1);
  }
  float ur = 1.f, ui = 0.f;
  if (l2_dir != nullptr) {
    ur = l2_dir[0];
    ui = l2_dir[1];
  }
  const float p = params[i];
  float add = 0.f;
  if (role == 0) {
    if (l1 != 0.f) add += l1 * (p > 0.f ? 1.f : (p < 0.f ? -1.f : 0.f));
    if (l2 != 0.f) add += 2.f * l2 * p * ur;
  } else {
    const float q = params[role == 1 ? i + 1 : i - 1];
    const float a = role == 1 ? p : q, b = role == 1 ? q : p;
    if (l1 != 0.f) {
      const float r = hypotf(a, b);
      if (r > 0.f) add += l1 * (p / r);
    }
    if (l2 != 0.f) add += role == 1 ? 2.f * l2 * (ur * a - ui * b) : -2.f * l2 * (ur * b + ui * a);
  }
  grads[i - lo] += add;
}

__global__ void step_advance_kernel(int* step_dev) { *step_dev += 1; }

hipError_t launch_step_advance(int* step_dev, hipStream_t st) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, st, step_dev);
  return hipGetLastError();
}

// has_dead / the dead layers' flat entries as merged ranges (MultiscaleKFourier's unused heads and last stage: SURVEY A.4 #3)
static void adam_dead_ranges(const NetDesc& nd, AdamArgs& aa) {
  aa.has_dead = 0;
  aa.n_dead = 0;
  int lo[2 * INR_MAX_LAYERS], hi[2 * INR_MAX_LAYERS], n = 0;
  for (int l = 0; l < nd.ND; ++l) {
    const LayerDesc& L = nd.L[l];
    if (L.live != 0) continue;
    aa.has_dead = 1;
    if (L.wn > 0) lo[n] = L.w_off, hi[n] = L.w_off + L.wn, ++n;
    if (L.bn > 0) lo[n] = L.b_off, hi[n] = L.b_off + L.bn, ++n;
  }
  for (int i = 1; i < n; ++i)  // by offset (insertion sort: a few dozen entries at most)
    for (int j = i; j > 0 && lo[j] < lo[j - 1]; --j) std::swap(lo[j], lo[j - 1]), std::swap(hi[j], hi[j - 1]);
  int m = 0;
  for (int i = 0; i < n; ++i) {
    if (m > 0 && lo[i] <= hi[m - 1]) {
      hi[m - 1] = std::max(hi[m - 1], hi[i]);
    } else {
      lo[m] = lo[i], hi[m] = hi[i], ++m;
    }
  }
  if (m > 8) {
    aa.n_dead = -1;
    return;
  }
  aa.n_dead = m;
  for (int i = 0; i < m; ++i) aa.dead_lo[i] = lo[i], aa.dead_hi[i] = hi[i];
}

hipError_t launch_adam_pack(const NetDesc& nd, float* params, const float* grads, float* m1, float* m2,
                            float* packed, const AdamArgs& aa_in, hipStream_t st) {
  AdamArgs aa = aa_in;
  aa.all_real = layers_real(nd, true);
  aa.flat_order = aa.all_real && layers_flat_order(nd);
  adam_dead_ranges(nd, aa);
  // large plain-layer networks (BASELINE config 4: 4.47 M entries): the update elementwise, then the images in image order
  // (INR_PACK_BY_IMAGE=0 / 1 forces the choice where both exist: the tests hold one against the other)
  const char* force = getenv("INR_PACK_BY_IMAGE");
  const bool big = force != nullptr ? force[0] == '1' : nd.P >= (1 << 18);
  bool by_image = aa.all_real && !nd.bf16 && !nd.rs && !nd.gabor && big;
  int slots = 0;
  for (int l = 0; l < nd.ND && by_image; ++l) {
    const LayerDesc& L = nd.L[l];
    by_image = L.ltype == LT_REAL && L.pf_off >= 0 && (L.pf_off & 3) == 0 && (L.pb_off < 0 || (L.pb_off & 3) == 0) &&
               (L.pbias_off & 3) == 0;
    slots = std::max(slots, L.Kpad8 * L.Mblk * 8 + (L.pb_off >= 0 ? L.Mpad8 * L.Kblk * 8 : 0) + L.Mblk * 8);
  }
  if (by_image) {
    if (aa.do_update)
      hipLaunchKernelGGL(adam_shard_kernel, dim3((nd.P + 255) / 256), dim3(256), 0, st, nd, params, grads, m1, m2, 0, nd.P,
                         aa);
    hipLaunchKernelGGL(pack_images_real_kernel, dim3((slots + 255) / 256, nd.ND), dim3(256), 0, st, nd, params, packed);
    return hipGetLastError();
  }
  const int grid = (nd.P + 255) / 256;
  hipLaunchKernelGGL(adam_pack_kernel, dim3(grid), dim3(256), 0, st, nd, params, grads, m1, m2, packed, aa);
  if (nd.gabor)
    hipLaunchKernelGGL(gabor_m2_kernel, dim3(nd.L[nd.mu0].M, nd.mfn_n + 1), dim3(64), 0, st, nd, params, packed);
  return hipGetLastError();
}

hipError_t launch_reg_grad(const NetDesc& nd, const float* params, float* grads, int lo, int hi, float l1, float l2,
                           const float* l2_dir, hipStream_t st) {
  if (hi <= lo || (l1 == 0.f && l2 == 0.f)) return hipSuccess;
  hipLaunchKernelGGL(reg_grad_kernel, dim3((hi - lo + 255) / 256), dim3(256), 0, st, nd, params, grads, lo, hi, l1, l2,
                     l2_dir);
  return hipGetLastError();
}

hipError_t launch_adam_shard(const NetDesc& nd, float* params, const float* grads_shard, float* m1, float* m2, int lo,
                             int hi, const AdamArgs& aa_in, hipStream_t st) {
  if (hi <= lo) return hipSuccess;
  AdamArgs aa = aa_in;
  aa.all_real = aa.flat_order = 0;
  adam_dead_ranges(nd, aa);
  hipLaunchKernelGGL(adam_shard_kernel, dim3((hi - lo + 255) / 256), dim3(256), 0, st, nd, params, grads_shard, m1, m2, lo,
                     hi, aa);
  return hipGetLastError();
}

// reduction (+ the Adam update when `adam` is given: one launch on the flat-layout fast path, two otherwise)
hipError_t launch_reduce_slabs_adam(const NetDesc& nd, const float* slabs, int n_blocks, float* grads, float* loss_out,
                                    float* params, float* m1, float* m2, float* packed, const AdamArgs& aa_in,
                                    hipStream_t st, SlabSplit split) {
  if (!(slabs_flat(nd, split) && ((split.lo3 | split.hi3) & 3) == 0 && !nd.gabor)) {
    hipError_t e = launch_reduce_slabs(nd, slabs, n_blocks, grads, loss_out, params, packed, st, split);
    if (e != hipSuccess) return e;
    return launch_adam_pack(nd, params, grads, m1, m2, packed, aa_in, st);
  }
  AdamArgs aa = aa_in;
  aa.all_real = 1;
  aa.flat_order = layers_flat_order(nd);
  adam_dead_ranges(nd, aa);
  const int grid = (nd.P + 255) / 256;
  hipLaunchKernelGGL(reduce_adam_real_kernel, dim3(grid + 1), dim3(256), 0, st, nd, slabs, n_blocks, grads, loss_out, split,
                     params, m1, m2, packed, aa);
  return hipGetLastError();
}

}  // namespace inr
