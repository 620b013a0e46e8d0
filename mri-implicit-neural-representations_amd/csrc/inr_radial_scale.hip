// inr_radial_scale.hip -- rows of an [n,2] field divided (or multiplied) by a continuous radial profile: the divisor of
// ring normalisation without its jumps at the ring edges (no reference counterpart).  The profile is
// piecewise linear on n_knots uniform knots that start at r_lo and lie 1 / inv_step apart, and constant beyond both ends.
// Per row, every line one correctly rounded fp32 operation:
//   s  = d - r_lo
//   u  = s * inv_step
//   u  = u < 0 ? 0 : (u > n_knots-1 ? n_knots-1 : u)
//   k  = min((int)u, n_knots - 2);   t = u - (float)k          (exact)
//   df = p[k+1] - p[k];   pr = t * df;   q = p[k] + pr
//   out = multiply ? in * q : in / q                           (both components)
// A row whose dist is NaN is copied bit for bit.  inr_mi355x/ringnorm.py::radial_scale_numpy is the same text in numpy.
//
// Rounding: hipcc contracts a + b*c into an FMA by default, which would merge `pr` and `q` into one rounding.  Contraction
// is switched off for this file (`#pragma clang fp contract(off)` below, ahead of every function) and the definition is
// written with plain operators.  The __f*_rn intrinsics are NOT a way to do this: the HIP headers define __fmul_rn and
// __fadd_rn as plain `x * y` and `x + y`, which contract like any other (measured: q off by 1-5 units in the last place
// against the numpy text).  The file is built with the library's flags, without any fast-math flag, and the division is
// `/`: correctly rounded, never a reciprocal-multiply.
//
// Mapping: inr_ring_scale.hip's -- a streaming kernel, 20 bytes per row; a block of 256 lanes takes tiles of 1024 rows,
// grid-strided over at most 2048 blocks; a lane takes 4 consecutive rows of a tile (dist one 16-B load, `in` two, `out`
// two 16-B stores when all three are 16-byte aligned; scalar accesses for the last partial group and for 8-byte aligned
// pointers).  A lane reads its rows before it writes them and no lane touches another's, so out == in is allowed.
//
// The table: staged in LDS once per block (4 * n_knots bytes of a 16 KB array, before the tile loop), gathered from there
// with two 4-byte reads per row.  The alternative is to gather p[k], p[k+1] from global memory through the vector cache.
// The choice rests on the worst case, not the common one.  On a grid the 256 rows of a wave-instruction lie along one
// k-space line and meet a handful of knots, and either path is invisible under 20 B/row of HBM traffic.  But rows in any
// other order (off-grid samples, a test's random radii) scatter the 64 addresses of a gather over the whole table: through
// the vector cache that is one pass per distinct line, up to 64 per instruction and 8 instructions per lane and tile, on
// the unit that the streaming loads and stores need as well; in LDS a 4-byte read is served in two 32-lane groups
// over 32 banks and a random pattern costs a few cycles.  The staging costs one coalesced pass over the table per block,
// at most 2048 * 16 KB from L2 against 20 B/row from HBM, and 16 KB of LDS still leaves 8 blocks (every wave slot) per CU.
// Only this path is built; its measured rate is in DESIGN.md 4.24.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

#pragma clang fp contract(off)

namespace inr {

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_LANE_ROWS = 4;
constexpr int RD_TILE_ROWS = RD_THREADS * RD_LANE_ROWS;
constexpr int RD_MAX_BLOCKS = 2048;

// VEC: dist, in and out are 16-byte aligned
template <bool VEC, bool MUL>
__global__ __launch_bounds__(RD_THREADS) void radial_scale_kernel(const float* __restrict__ dist, const float* in, float* out,
                                                                  const unsigned n, const unsigned tiles,
                                                                  const float* __restrict__ profile, const int n_knots,
                                                                  const float r_lo, const float inv_step) {
  __shared__ float tab[RADIAL_KNOTS_MAX];
  for (int i = threadIdx.x; i < n_knots; i += RD_THREADS) tab[i] = profile[i];
  __syncthreads();
  const float u_hi = (float)(n_knots - 1);
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned r = tile * (unsigned)RD_TILE_ROWS + threadIdx.x * RD_LANE_ROWS;  // < 2^31 + 1024
    const bool whole = VEC && r + RD_LANE_ROWS <= n;
    float d[RD_LANE_ROWS], v[2 * RD_LANE_ROWS];
    if (whole) {
      const float4 d4 = *reinterpret_cast<const float4*>(dist + r);
      const float4 v0 = *reinterpret_cast<const float4*>(in + 2 * (size_t)r);
      const float4 v1 = *reinterpret_cast<const float4*>(in + 2 * (size_t)r + 4);
      d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
      v[0] = v0.x, v[1] = v0.y, v[2] = v0.z, v[3] = v0.w, v[4] = v1.x, v[5] = v1.y, v[6] = v1.z, v[7] = v1.w;
    } else {
#pragma unroll
      for (int j = 0; j < RD_LANE_ROWS; ++j) {
        const bool have = r + j < n;  // rows past the end pass through as NaN rows and are never stored
        d[j] = have ? dist[r + j] : NAN;
        v[2 * j] = have ? in[2 * (size_t)(r + j)] : 0.f;
        v[2 * j + 1] = have ? in[2 * (size_t)(r + j) + 1] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < RD_LANE_ROWS; ++j) {
      const bool is_nan = d[j] != d[j];
      const float s = d[j] - r_lo;
      float u = s * inv_step;
      u = u < 0.f ? 0.f : (u > u_hi ? u_hi : u);
      u = is_nan ? 0.f : u;  // the row is copied; keeps the index below inside the table
      int k = (int)u;        // 0 <= u <= n_knots - 1 <= 4095: exact truncation
      k = k < n_knots - 2 ? k : n_knots - 2;
      const float t = u - (float)k;
      const float p0 = tab[k], p1 = tab[k + 1];
      const float df = p1 - p0;
      const float pr = t * df;
      const float q = p0 + pr;
      const float a0 = MUL ? v[2 * j] * q : v[2 * j] / q;
      const float a1 = MUL ? v[2 * j + 1] * q : v[2 * j + 1] / q;
      v[2 * j] = is_nan ? v[2 * j] : a0;
      v[2 * j + 1] = is_nan ? v[2 * j + 1] : a1;
    }
    if (whole) {
      *reinterpret_cast<float4*>(out + 2 * (size_t)r) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(out + 2 * (size_t)r + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
      for (int j = 0; j < RD_LANE_ROWS; ++j)
        if (r + j < n) {
          out[2 * (size_t)(r + j)] = v[2 * j];
          out[2 * (size_t)(r + j) + 1] = v[2 * j + 1];
        }
    }
  }
}

template <bool VEC, bool MUL>
void launch(unsigned blocks, hipStream_t st, const float* dist, const float* in, float* out, unsigned n, unsigned tiles,
            const float* profile, int n_knots, float r_lo, float inv_step) {
  hipLaunchKernelGGL((radial_scale_kernel<VEC, MUL>), dim3(blocks), dim3(RD_THREADS), 0, st, dist, in, out, n, tiles,
                     profile, n_knots, r_lo, inv_step);
}

}  // namespace

hipError_t launch_radial_scale(const float* dist, const float* in, float* out, long long n, const float* profile,
                               int n_knots, float r_lo, float inv_step, bool multiply, hipStream_t st) {
  const unsigned tiles = (unsigned)((n + RD_TILE_ROWS - 1) / RD_TILE_ROWS);
  const unsigned blocks = tiles < (unsigned)RD_MAX_BLOCKS ? tiles : (unsigned)RD_MAX_BLOCKS;
  const bool vec = (((uintptr_t)dist | (uintptr_t)in | (uintptr_t)out) & 15u) == 0;
  auto* f = vec ? (multiply ? launch<true, true> : launch<true, false>) : (multiply ? launch<false, true> : launch<false, false>);
  f(blocks, st, dist, in, out, (unsigned)n, tiles, profile, n_knots, r_lo, inv_step);
  return hipGetLastError();
}

}  // namespace inr
