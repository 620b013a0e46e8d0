// inr_grid.hip -- rows of a coordinate grid, made on the device a chunk at a time (replaces create_coords,
// data/utils.py:98-108, and its upload).  Row r = (k H + y) W + x of the flattened (k, y, x) grid is
//   (v(coils[k]; -1, 1, coils_total), v(y; y0, y1, H), v(x; x0, x1, W)),   dist = sqrt(y^2 + x^2),
//   v(i; a, b, n) = a                           when n == 1,
//                   a + step * i                for i < n / 2,
//                   b - step * (n - 1 - i)      for the rest,      step = (b - a) / (n - 1),
// in fp32 with every operation rounded on its own: the host divides (IEEE), the device multiplies and adds under
// `#pragma clang fp contract(off)` -- the _rn intrinsics are plain operators in HIP's headers and would still be fused
// into FMAs once inlined.  inr_mi355x/grid.py::grid_rows_numpy is the same text in numpy.
//
// Mapping: a block of 256 lanes makes 1024 consecutive rows, a lane 4 of them -- one division of the row index into
// (k, y, x), then three carries.  A row is 12 B, so the lane's 4 rows are three whole 16-B words; they pass through LDS
// so that lane t of the block then stores words t, t + 256 and t + 512 of the block's 12 KiB: every store instruction of
// a wave writes 1 KiB of consecutive bytes.  dist is one 16-B store per lane straight from registers.  Write-only,
// 16 B per row; a buffer that is not 16-byte aligned takes the same kernel with 4-byte stores.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

#pragma clang fp contract(off)  // a + step * i is two roundings, by definition

namespace inr {

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_LANE_ROWS = 4;
constexpr int GR_BLOCK_ROWS = GR_THREADS * GR_LANE_ROWS;

__device__ inline float axis_value(int i, float a, float b, int n, float step) {
  if (n == 1) return a;
  if (i < n / 2) return a + step * (float)i;
  return b - step * (float)(n - 1 - i);
}

// VEC: coords and dist are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(GR_THREADS) void grid_rows_kernel(const GridArgs g, const unsigned n_rows,
                                                                float* __restrict__ coords, float* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float stage[GR_BLOCK_ROWS * 3];
  const unsigned t = threadIdx.x;
  const unsigned block_row = blockIdx.x * (unsigned)GR_BLOCK_ROWS;  // < n_rows < 2^31
  const unsigned r = block_row + t * GR_LANE_ROWS;                  // the lane's first row of the chunk
  if (r < n_rows) {
    // row_lo + r as (k, y, x): the host split row_lo, the carries of r stay below 2^32
    const unsigned xt = g.x_lo + r;
    int x = (int)(xt % (unsigned)g.W);
    const unsigned yt = g.y_lo + xt / (unsigned)g.W;
    int y = (int)(yt % (unsigned)g.H);
    int k = (int)(g.k_lo + yt / (unsigned)g.H);
    float c[GR_LANE_ROWS * 3], d[GR_LANE_ROWS];
#pragma unroll
    for (int j = 0; j < GR_LANE_ROWS; ++j) {
      // rows past the chunk's end may step past the last coil: they are computed and never stored
      const int coil = g.coils[k < g.n_coils ? k : g.n_coils - 1];
      const float vy = axis_value(y, g.wy0, g.wy1, g.H, g.step_y);
      const float vx = axis_value(x, g.wx0, g.wx1, g.W, g.step_x);
      c[3 * j + 0] = axis_value(coil, -1.f, 1.f, g.coils_total, g.step_z);
      c[3 * j + 1] = vy;
      c[3 * j + 2] = vx;
      d[j] = sqrtf(vy * vy + vx * vx);  // IEEE: hipcc rounds fp32 sqrt correctly by default (__fsqrt_rn is the 1-ulp native one)
      if (++x == g.W) {
        x = 0;
        if (++y == g.H) {
          y = 0;
          ++k;
        }
      }
    }
    float4* s4 = reinterpret_cast<float4*>(stage + t * (GR_LANE_ROWS * 3));
    s4[0] = make_float4(c[0], c[1], c[2], c[3]);
    s4[1] = make_float4(c[4], c[5], c[6], c[7]);
    s4[2] = make_float4(c[8], c[9], c[10], c[11]);
    if (dist != nullptr) {
      if (VEC && r + GR_LANE_ROWS <= n_rows) {
        *reinterpret_cast<float4*>(dist + r) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
#pragma unroll
        for (int j = 0; j < GR_LANE_ROWS; ++j)
          if (r + j < n_rows) dist[r + j] = d[j];
      }
    }
  }
  __syncthreads();
  const unsigned left = n_rows - block_row;
  const unsigned nf = 3u * (left < (unsigned)GR_BLOCK_ROWS ? left : (unsigned)GR_BLOCK_ROWS);  // floats this block owns
  float* out = coords + (size_t)block_row * 3;
  if (VEC) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const unsigned f = 4u * (t + p * GR_THREADS);
      if (f + 4 <= nf) {
        *reinterpret_cast<float4*>(out + f) = *reinterpret_cast<const float4*>(stage + f);
      } else {
        for (unsigned e = f; e < nf && e < f + 4; ++e) out[e] = stage[e];
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < GR_LANE_ROWS * 3; ++p) {
      const unsigned f = t + p * GR_THREADS;
      if (f < nf) out[f] = stage[f];
    }
  }
}

}  // namespace

hipError_t launch_grid_rows(const GridArgs& g, long long n_rows, float* coords, float* dist, hipStream_t st) {
  const unsigned blocks = (unsigned)((n_rows + GR_BLOCK_ROWS - 1) / GR_BLOCK_ROWS);
  const bool vec = (((uintptr_t)coords | (uintptr_t)dist) & 15u) == 0;
  if (vec)
    hipLaunchKernelGGL(grid_rows_kernel<true>, dim3(blocks), dim3(GR_THREADS), 0, st, g, (unsigned)n_rows, coords, dist);
  else
    hipLaunchKernelGGL(grid_rows_kernel<false>, dim3(blocks), dim3(GR_THREADS), 0, st, g, (unsigned)n_rows, coords, dist);
  return hipGetLastError();
}

}  // namespace inr
