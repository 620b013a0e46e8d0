// inr_shuffle.hip -- the keyed row permutation of a shuffled epoch (gfx950)
#include "inr_epoch_rows.h"

namespace inr {

// One thread per output row of the keyed permutation shuffle_order; the gather and the batch counts are epoch_row
// (inr_epoch_rows.h).
__global__ __launch_bounds__(256) void shuffle_epoch_kernel(const ShuffleKeys sk, unsigned n, unsigned bs,
                                                            const float* __restrict__ coords,
                                                            const float* __restrict__ gt,
                                                            const float* __restrict__ dist,
                                                            const uint8_t* __restrict__ mask,
                                                            float* __restrict__ coords_out, float* __restrict__ gt_out,
                                                            float* __restrict__ dist_out, uint8_t* __restrict__ mask_out,
                                                            int* __restrict__ batch_counts,
                                                            long long* __restrict__ order_out) {
  const unsigned long long jj = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = jj < n;
  const unsigned j = (unsigned)jj;
  const size_t i = live ? shuffle_order(sk, j, n) : 0;  // < n by construction
  epoch_row(jj, n, bs, live, i, coords, gt, dist, mask, coords_out, gt_out, dist_out, mask_out, batch_counts, order_out);
}

hipError_t launch_shuffle_epoch(const ShuffleKeys& sk, long long n, long long bs, const float* coords, const float* gt,
                                const float* dist, const uint8_t* mask, float* coords_out, float* gt_out, float* dist_out,
                                uint8_t* mask_out, int* batch_counts, long long* order_out, hipStream_t st) {
  const hipError_t e = epoch_counts_begin(batch_counts, n, &bs, st);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(shuffle_epoch_kernel, dim3(grid), dim3(256), 0, st, sk, (unsigned)n,
                     (unsigned)bs, coords, gt, dist, mask, coords_out, gt_out, dist_out, mask_out,
                     batch_counts, order_out);
  return hipGetLastError();
}

}  // namespace inr
