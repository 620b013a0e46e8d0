// inr_reduce.h -- the block reduction of the helper kernels: a fixed-order tree over the N lanes of a workgroup through
// LDS, s = N/2 ... 1, red[t] = op(red[t], red[t + s]).  The shape is part of every result's bits: do not change it.
#pragma once
#include <hip/hip_runtime.h>

namespace inr {

struct Sum {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct MaxF {
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct MinF {
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
};

// the tree, ending at the barrier after its last step: every lane may read the result, nobody may write `red` again
// (kernels that store the result from lane 0 and are done)
template <int N, typename T, typename Op>
__device__ __forceinline__ T block_reduce_once(T v, T* red, Op op) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = op(red[t], red[t + s]);
    __syncthreads();
  }
  return red[0];
}

// ... and with a trailing barrier: `red` may be reused afterwards
template <int N, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* red, Op op) {
  const T r = block_reduce_once<N>(v, red, op);
  __syncthreads();
  return r;
}

}  // namespace inr
