// inr_epoch_rows.h -- what the two kernels that fill an epoch's buffers share (inr_shuffle.hip: every row once, in a keyed
// order; inr_sample.hip: rows drawn by weight): the keyed bijection and the gather of one output row with its count.
#pragma once
#include "inr_device.h"
#include "inr_aux.h"

namespace inr {

// ---------------------------------------------------------------------------------------------
// Shuffled epochs: output row j of the epoch is input row order(j), a keyed bijection of [0, 2^(2h))
// -- a balanced Feistel network of SHUFFLE_ROUNDS rounds over two h-bit halves, round function
// (MIX(R ^ K_r) >> 16) & (2^h - 1) -- walked until it lands in [0, n).  32-bit integer arithmetic only, so
// inr_mi355x/shuffle.py::epoch_order gives the same integers.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned shuffle_order(const ShuffleKeys& sk, unsigned j, unsigned n) {
  const unsigned half = (1u << sk.h) - 1u;
  unsigned x = j;
  do {
    unsigned l = x >> sk.h, r = x & half;
#pragma unroll
    for (int i = 0; i < SHUFFLE_ROUNDS; ++i) {
      const unsigned t = l ^ ((shuffle_mix(r ^ sk.k[i]) >> 16) & half);
      l = r;
      r = t;
    }
    x = (l << sk.h) | r;
  } while (x >= n);
  return x;
}

// Output row jj (of n_out; one thread per output row, 256-thread blocks) takes source row i: the writes of a wave are
// contiguous (12 / 8 / 4 / 1 / 8 bytes per lane), the reads are single rows anywhere in the source.
// batch_counts (zeroed by the launcher on the same stream) takes one integer atomic per wave whose 64 rows lie in one
// batch, one per lane in the wave that straddles a batch end: integer sums, exact in any order.  Every lane of the
// block calls this (the ballot below is wave-wide); ``live`` = jj < n_out, and i is read only when it is set.
__device__ __forceinline__ void epoch_row(unsigned long long jj, unsigned n_out, unsigned bs, bool live, size_t i,
                                          const float* __restrict__ coords, const float* __restrict__ gt,
                                          const float* __restrict__ dist, const uint8_t* __restrict__ mask,
                                          float* __restrict__ coords_out, float* __restrict__ gt_out,
                                          float* __restrict__ dist_out, uint8_t* __restrict__ mask_out,
                                          int* __restrict__ batch_counts, long long* __restrict__ order_out) {
  const unsigned j = (unsigned)jj;
  int sampled = 0;
  if (live) {
    const size_t o = j;
    if (coords_out != nullptr) {
      const float c0 = coords[3 * i], c1 = coords[3 * i + 1], c2 = coords[3 * i + 2];
      coords_out[3 * o] = c0;
      coords_out[3 * o + 1] = c1;
      coords_out[3 * o + 2] = c2;
    }
    if (gt_out != nullptr)
      reinterpret_cast<float2*>(gt_out)[o] = reinterpret_cast<const float2*>(gt)[i];
    if (dist_out != nullptr) dist_out[o] = dist[i];
    sampled = 1;
    if (mask != nullptr) {
      const uint8_t m = mask[i];
      if (mask_out != nullptr) mask_out[o] = m;
      sampled = m != 0 ? 1 : 0;
    }
    if (order_out != nullptr) order_out[o] = (long long)i;
  }
  if (batch_counts != nullptr) {
    // a wave's rows are [w0, w0 + 64): one batch unless a batch end falls inside (wave-uniform test)
    const unsigned long long w0 = jj - (threadIdx.x & 63);
    const unsigned long long wl = (w0 + 63 < n_out ? w0 + 63 : (unsigned long long)n_out - 1);
    if (w0 < n_out) {
      const unsigned b0 = (unsigned)(w0 / bs), b1 = (unsigned)(wl / bs);
      if (b0 == b1) {
        const int cnt = __popcll(__ballot(sampled != 0));
        if ((threadIdx.x & 63) == 0 && cnt != 0) atomicAdd(batch_counts + b0, cnt);
      } else if (live && sampled) {
        atomicAdd(batch_counts + j / bs, 1);
      }
    }
  }
}

// zeroes batch_counts on the stream and gives the batch size the kernel divides by (1 without counts)
inline hipError_t epoch_counts_begin(int* batch_counts, long long n_out, long long* bs, hipStream_t st) {
  if (batch_counts == nullptr) {
    *bs = 1;
    return hipSuccess;
  }
  const long long nb = (n_out + *bs - 1) / *bs;
  if (*bs > n_out) *bs = n_out;
  return hipMemsetAsync(batch_counts, 0, (size_t)nb * sizeof(int), st);
}

}  // namespace inr
