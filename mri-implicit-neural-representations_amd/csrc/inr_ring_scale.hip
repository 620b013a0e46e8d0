// inr_ring_scale.hip -- rows of an [n,2] field divided by the divisor of the ring their radius lies in (DESIGN.md 4.22;
// the reference's scale_space, train_variations/train_normalize_per_bucket.py:20-27).  Row i belongs to ring r iff
// radii[r] <= dist[i] < radii[r+1] in fp32, lower end included, upper end excluded; both components of such a row become
// in / divisors[r], one correctly rounded fp32 division each (this file is built without any fast-math flag and writes
// `/`: never a reciprocal-multiply).  A row in no ring -- below radii[0], at or above the last radius, NaN -- is copied
// bit for bit.  The radii do not decrease, so the ring of a row is (number of radii <= dist) - 1, which is what
// np.searchsorted(radii, dist, side="right") - 1 gives; equal neighbours make an empty ring and a row at that radius
// falls into the next one.  inr_mi355x/ringnorm.py::ring_scale_numpy is the same text in numpy.
//
// Mapping: a streaming kernel, 20 bytes per row.  A block of 256 lanes takes tiles of 1024 rows, grid-strided over at
// most 2048 blocks; a lane takes 4 consecutive rows of a tile -- dist is one 16-B load, `in` two, `out` two 16-B stores.
// The table travels as kernel arguments (scalar loads); the walk over the radii is wave-uniform and ends at the first
// radius above every dist of the wave.  A lane reads its rows before it writes them and no lane touches another's, so
// out == in is allowed.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

namespace inr {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LANE_ROWS = 4;
constexpr int RS_TILE_ROWS = RS_THREADS * RS_LANE_ROWS;
constexpr int RS_MAX_BLOCKS = 2048;

// VEC: dist, in and out are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void ring_scale_kernel(const RingArgs a, const float* __restrict__ dist,
                                                                const float* in, float* out, const unsigned n,
                                                                const unsigned tiles) {
  const int K = a.n_rings;
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned r = tile * (unsigned)RS_TILE_ROWS + threadIdx.x * RS_LANE_ROWS;  // < 2^31 + 1024
    const bool whole = VEC && r + RS_LANE_ROWS <= n;
    float d[RS_LANE_ROWS], v[2 * RS_LANE_ROWS];
    if (whole) {
      const float4 d4 = *reinterpret_cast<const float4*>(dist + r);
      const float4 v0 = *reinterpret_cast<const float4*>(in + 2 * (size_t)r);
      const float4 v1 = *reinterpret_cast<const float4*>(in + 2 * (size_t)r + 4);
      d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
      v[0] = v0.x, v[1] = v0.y, v[2] = v0.z, v[3] = v0.w, v[4] = v1.x, v[5] = v1.y, v[6] = v1.z, v[7] = v1.w;
    } else {
#pragma unroll
      for (int j = 0; j < RS_LANE_ROWS; ++j) {
        const bool have = r + j < n;  // rows past the end are in no ring (NaN compares false) and are never stored
        d[j] = have ? dist[r + j] : NAN;
        v[2 * j] = have ? in[2 * (size_t)(r + j)] : 0.f;
        v[2 * j + 1] = have ? in[2 * (size_t)(r + j) + 1] : 0.f;
      }
    }
    float div[RS_LANE_ROWS];
    bool hit[RS_LANE_ROWS];
#pragma unroll
    for (int j = 0; j < RS_LANE_ROWS; ++j) div[j] = 1.f, hit[j] = false;
    for (int b = 0; b <= K; ++b) {
      const float lo = a.radii[b];
      const float dv = b < K ? a.divisors[b] : 1.f;
      bool any = false;
#pragma unroll
      for (int j = 0; j < RS_LANE_ROWS; ++j) {
        const bool ge = d[j] >= lo;
        any |= ge;
        div[j] = ge ? dv : div[j];
        hit[j] = ge ? b < K : hit[j];  // at or above the last radius: in no ring again
      }
      if (__ballot(any) == 0ull) break;  // wave-uniform; the radii do not decrease
    }
#pragma unroll
    for (int j = 0; j < RS_LANE_ROWS; ++j) {
      const float q0 = v[2 * j] / div[j], q1 = v[2 * j + 1] / div[j];
      v[2 * j] = hit[j] ? q0 : v[2 * j];
      v[2 * j + 1] = hit[j] ? q1 : v[2 * j + 1];
    }
    if (whole) {
      *reinterpret_cast<float4*>(out + 2 * (size_t)r) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(out + 2 * (size_t)r + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
      for (int j = 0; j < RS_LANE_ROWS; ++j)
        if (r + j < n) {
          out[2 * (size_t)(r + j)] = v[2 * j];
          out[2 * (size_t)(r + j) + 1] = v[2 * j + 1];
        }
    }
  }
}

}  // namespace

hipError_t launch_ring_scale(const RingArgs& a, const float* dist, const float* in, float* out, long long n,
                             hipStream_t st) {
  const unsigned tiles = (unsigned)((n + RS_TILE_ROWS - 1) / RS_TILE_ROWS);
  const unsigned blocks = tiles < (unsigned)RS_MAX_BLOCKS ? tiles : (unsigned)RS_MAX_BLOCKS;
  const bool vec = (((uintptr_t)dist | (uintptr_t)in | (uintptr_t)out) & 15u) == 0;
  if (vec)
    hipLaunchKernelGGL(ring_scale_kernel<true>, dim3(blocks), dim3(RS_THREADS), 0, st, a, dist, in, out, (unsigned)n, tiles);
  else
    hipLaunchKernelGGL(ring_scale_kernel<false>, dim3(blocks), dim3(RS_THREADS), 0, st, a, dist, in, out, (unsigned)n, tiles);
  return hipGetLastError();
}

}  // namespace inr
