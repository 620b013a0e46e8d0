// inr_display.hip -- the pictures and the per-coil table of the validation epoch (train.py:221-238; models/utils.py:254-287)
// on gfx950.  Three entry points, all HBM-bound, no atomics, no host synchronisation, nothing allocated; every reduction
// is a fixed-order tree inside a block followed by a fixed-order fold of the per-block partials, so results are bitwise
// reproducible.
//
//   k-space display (save_im, is_kspace branch, :262-267, in fp32 as there):
//     g = rss_c(complex_abs(z_c))  [z = coils - minus when an error picture is asked for];  g *= expm1(sf) / max g;
//     g = log1p(g);  g /= max g.   Three launches: RSS + block maxima | fold, scale, log1p + block maxima | fold, divide.
//     max propagates NaN as torch.max does; an all-zero input is 0 * (expm1(sf) / 0) = NaN everywhere, as the reference's.
//   gray8 (what plt.imsave(..., cmap="gray") stores in the R channel of its PNG):
//     n = (x - vmin) / (vmax - vmin) in fp32 (vmin / vmax: the finite extrema of the picture unless given; vmax == vmin
//     gives n = 0), index min(floor(256 n), 255) (below vmin: 0, above vmax: 255), byte = lut[index] -- matplotlib's table
//     is not the identity, the host uploads it.  Non-finite pixels are masked by matplotlib and come out as byte 0.
//     Two launches (one when vmin / vmax are given).
//   coil statistics (stats_per_coil, :274-283): mean, unbiased std, max, min over the 2 H W values of each coil,
//     accumulated in fp64 in two passes (sum -> mean; sum of squared deviations, extrema) plus a one-block-per-coil fold.
#include <hip/hip_runtime.h>
#include <cmath>
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_MAX_BLOCKS = 512;      // per-pixel passes
constexpr int DP_COIL_MAX_BLOCKS = 256;  // blocks per coil of the statistics passes

inline int dp_blocks(long long n, int cap) {
  const long long b = (n + DP_THREADS - 1) / DP_THREADS;
  return (int)(b < cap ? b : cap);
}

// torch.max: a NaN anywhere is the result
struct NanMaxF {
  __device__ float operator()(float a, float b) const { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
};

// fold of G per-block partials, the same value in every lane of every block
template <typename Op>
__device__ float fold_partials(const float* __restrict__ part, int G, float init, float* red, Op op) {
  float v = init;
  for (int i = threadIdx.x; i < G; i += DP_THREADS) v = op(v, part[i]);
  return block_reduce<DP_THREADS>(v, red, op);
}

// ---- k-space display ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DP_THREADS) void display_rss_kernel(const float2* __restrict__ coils,
                                                                  const float2* __restrict__ minus, int C, long long n,
                                                                  float* __restrict__ out, float* __restrict__ part) {
  __shared__ float red[DP_THREADS];
  const NanMaxF nmax;
  float mx = -INFINITY;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n; p += stride) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      float2 z = coils[(long long)c * n + p];
      if (minus != nullptr) {
        const float2 w = minus[(long long)c * n + p];
        z.x = __fsub_rn(z.x, w.x);
        z.y = __fsub_rn(z.y, w.y);
      }
      const float m = __fsqrt_rn(__fadd_rn(__fmul_rn(z.x, z.x), __fmul_rn(z.y, z.y)));  // complex_abs
      s = __fadd_rn(s, __fmul_rn(m, m));                                                 // rss: sum_c |z|^2
    }
    const float r = __fsqrt_rn(s);
    out[p] = r;
    mx = nmax(mx, r);
  }
  mx = block_reduce<DP_THREADS>(mx, red, nmax);
  if (threadIdx.x == 0) part[blockIdx.x] = mx;
}

// out *= em / max;  out = log1p(out)   (em = expm1(sf), rounded to fp32 on the host)
__global__ __launch_bounds__(DP_THREADS) void display_log_kernel(float* __restrict__ out, long long n, float em,
                                                                  const float* __restrict__ part_in, int G,
                                                                  float* __restrict__ part_out) {
  __shared__ float red[DP_THREADS];
  const NanMaxF nmax;
  const float scale = __fdiv_rn(em, fold_partials(part_in, G, -INFINITY, red, nmax));
  float mx = -INFINITY;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n; p += stride) {
    const float v = log1pf(__fmul_rn(out[p], scale));
    out[p] = v;
    mx = nmax(mx, v);
  }
  mx = block_reduce<DP_THREADS>(mx, red, nmax);
  if (threadIdx.x == 0) part_out[blockIdx.x] = mx;
}

__global__ __launch_bounds__(DP_THREADS) void display_unit_kernel(float* __restrict__ out, long long n,
                                                                   const float* __restrict__ part_in, int G) {
  __shared__ float red[DP_THREADS];
  const float mx = fold_partials(part_in, G, -INFINITY, red, NanMaxF());
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n; p += stride) out[p] = __fdiv_rn(out[p], mx);
}

// ---- gray8 ----------------------------------------------------------------------------------------------------------
__device__ inline bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }  // false for NaN and +-inf

// part: [2][G] = min, max of the finite pixels of each block
__global__ __launch_bounds__(DP_THREADS) void gray_extrema_kernel(const float* __restrict__ img, long long n, int take_abs,
                                                                   float* __restrict__ part) {
  __shared__ float red[DP_THREADS];
  float mn = INFINITY, mx = -INFINITY;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n; p += stride) {
    float x = img[p];
    if (take_abs) x = fabsf(x);
    if (finite_f(x)) {
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
  }
  mn = block_reduce<DP_THREADS>(mn, red, MinF());
  mx = block_reduce<DP_THREADS>(mx, red, MaxF());
  if (threadIdx.x == 0) {
    part[blockIdx.x] = mn;
    part[gridDim.x + blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(DP_THREADS) void gray_quantise_kernel(const float* __restrict__ img, long long n, int take_abs,
                                                                    const float* __restrict__ part, int G, float vmin,
                                                                    float vmax, const unsigned char* __restrict__ lut,
                                                                    unsigned char* __restrict__ out,
                                                                    float* __restrict__ norm_out) {
  __shared__ float red[DP_THREADS];
  if (part != nullptr) {  // the picture's own extrema (uniform over the grid)
    vmin = fold_partials(part, G, INFINITY, red, MinF());
    vmax = fold_partials(part + G, G, -INFINITY, red, MaxF());
  }
  const float range = __fsub_rn(vmax, vmin);
  const bool flat = vmax == vmin;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n; p += stride) {
    float x = img[p];
    if (take_abs) x = fabsf(x);
    unsigned char b = 0;
    float nv = NAN;
    if (finite_f(x)) {
      nv = flat ? 0.f : __fdiv_rn(__fsub_rn(x, vmin), range);
      const float t = __fmul_rn(nv, 256.f);  // exact
      int i = t < 0.f ? 0 : (t >= 255.f ? 255 : (int)t);  // (a NaN range leaves t NaN: index 255 is never read, i = 0 below)
      if (t != t) i = 0;
      b = lut[i];
    }
    out[p] = b;
    if (norm_out != nullptr) norm_out[p] = nv;
  }
}

// ---- coil statistics ------------------------------------------------------------------------------------------------
// grid (G, C); part_sum [C][G]
__global__ __launch_bounds__(DP_THREADS) void coil_sum_kernel(const float2* __restrict__ coils, long long n2,
                                                               double* __restrict__ part_sum) {
  __shared__ double red[DP_THREADS];
  const float2* base = coils + (long long)blockIdx.y * n2;
  double s = 0.0;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n2; p += stride) {
    const float2 z = base[p];
    s += (double)z.x;
    s += (double)z.y;
  }
  s = block_reduce<DP_THREADS>(s, red, Sum());
  if (threadIdx.x == 0) part_sum[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__device__ double coil_mean(const double* __restrict__ part_sum, int G, long long n2, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < G; i += DP_THREADS) s += part_sum[i];
  return block_reduce<DP_THREADS>(s, red, Sum()) / (2.0 * (double)n2);
}

// part_dev [3][C][G] = sum of squared deviations from the coil's mean, max, min
__global__ __launch_bounds__(DP_THREADS) void coil_dev_kernel(const float2* __restrict__ coils, long long n2,
                                                               const double* __restrict__ part_sum,
                                                               double* __restrict__ part_dev) {
  __shared__ double red[DP_THREADS];
  __shared__ float fred[DP_THREADS];
  const int G = gridDim.x, C = gridDim.y, c = blockIdx.y;
  const double mean = coil_mean(part_sum + (long long)c * G, G, n2, red);
  const float2* base = coils + (long long)c * n2;
  double m2 = 0.0;
  float mx = -INFINITY, mn = INFINITY;
  const long long stride = (long long)G * DP_THREADS;
  for (long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x; p < n2; p += stride) {
    const float2 z = base[p];
    const double a = (double)z.x - mean, b = (double)z.y - mean;
    m2 += a * a;
    m2 += b * b;
    mx = fmaxf(mx, fmaxf(z.x, z.y));
    mn = fminf(mn, fminf(z.x, z.y));
  }
  m2 = block_reduce<DP_THREADS>(m2, red, Sum());
  mx = block_reduce<DP_THREADS>(mx, fred, MaxF());
  mn = block_reduce<DP_THREADS>(mn, fred, MinF());
  if (threadIdx.x == 0) {
    const long long o = (long long)c * G + blockIdx.x, cg = (long long)C * G;
    part_dev[o] = m2;
    part_dev[cg + o] = (double)mx;
    part_dev[2 * cg + o] = (double)mn;
  }
}

// one block per coil: stats[c] = mean, std (n - 1), max, min
__global__ __launch_bounds__(DP_THREADS) void coil_final_kernel(const double* __restrict__ part_sum,
                                                                 const double* __restrict__ part_dev, int G, long long n2,
                                                                 double* __restrict__ stats) {
  __shared__ double red[DP_THREADS];
  __shared__ float fred[DP_THREADS];
  const int C = gridDim.x, c = blockIdx.x;
  const long long cg = (long long)C * G, o = (long long)c * G;
  const double mean = coil_mean(part_sum + o, G, n2, red);
  double m2 = 0.0;
  float mx = -INFINITY, mn = INFINITY;
  for (int i = threadIdx.x; i < G; i += DP_THREADS) {
    m2 += part_dev[o + i];
    mx = fmaxf(mx, (float)part_dev[cg + o + i]);
    mn = fminf(mn, (float)part_dev[2 * cg + o + i]);
  }
  m2 = block_reduce<DP_THREADS>(m2, red, Sum());
  mx = block_reduce<DP_THREADS>(mx, fred, MaxF());
  mn = block_reduce<DP_THREADS>(mn, fred, MinF());
  if (threadIdx.x == 0) {
    stats[4 * c + 0] = mean;
    stats[4 * c + 1] = sqrt(m2 / (2.0 * (double)n2 - 1.0));
    stats[4 * c + 2] = (double)mx;
    stats[4 * c + 3] = (double)mn;
  }
}

}  // namespace

long long kspace_display_scratch_floats(long long H, long long W) { return 2LL * dp_blocks(H * W, DP_MAX_BLOCKS); }

hipError_t launch_kspace_display(const float* coils, const float* minus, int C, int H, int W, float expm1_sf, float* out,
                                 float* scratch, hipStream_t st) {
  const long long n = (long long)H * W;
  const int G = dp_blocks(n, DP_MAX_BLOCKS);
  hipLaunchKernelGGL(display_rss_kernel, dim3(G), dim3(DP_THREADS), 0, st, reinterpret_cast<const float2*>(coils),
                     reinterpret_cast<const float2*>(minus), C, n, out, scratch);
  hipLaunchKernelGGL(display_log_kernel, dim3(G), dim3(DP_THREADS), 0, st, out, n, expm1_sf, scratch, G, scratch + G);
  hipLaunchKernelGGL(display_unit_kernel, dim3(G), dim3(DP_THREADS), 0, st, out, n, scratch + G, G);
  return hipGetLastError();
}

long long gray8_scratch_floats(long long H, long long W) { return 2LL * dp_blocks(H * W, DP_MAX_BLOCKS); }

hipError_t launch_gray8(const float* img, int H, int W, int take_abs, int has_range, float vmin, float vmax,
                        const unsigned char* lut, unsigned char* out, float* norm_out, float* scratch, hipStream_t st) {
  const long long n = (long long)H * W;
  const int G = dp_blocks(n, DP_MAX_BLOCKS);
  if (!has_range)
    hipLaunchKernelGGL(gray_extrema_kernel, dim3(G), dim3(DP_THREADS), 0, st, img, n, take_abs, scratch);
  hipLaunchKernelGGL(gray_quantise_kernel, dim3(G), dim3(DP_THREADS), 0, st, img, n, take_abs,
                     has_range ? (const float*)nullptr : scratch, G, vmin, vmax, lut, out, norm_out);
  return hipGetLastError();
}

long long coil_stats_scratch_doubles(long long C, long long H, long long W) {
  return 4LL * C * dp_blocks(H * W, DP_COIL_MAX_BLOCKS);
}

hipError_t launch_coil_stats(const float* coils, int C, int H, int W, double* stats, double* scratch, hipStream_t st) {
  const long long n2 = (long long)H * W;  // (re, im) pairs per coil
  const int G = dp_blocks(n2, DP_COIL_MAX_BLOCKS);
  double* part_sum = scratch;
  double* part_dev = scratch + (long long)C * G;
  const float2* z = reinterpret_cast<const float2*>(coils);
  hipLaunchKernelGGL(coil_sum_kernel, dim3(G, C), dim3(DP_THREADS), 0, st, z, n2, part_sum);
  hipLaunchKernelGGL(coil_dev_kernel, dim3(G, C), dim3(DP_THREADS), 0, st, z, n2, part_sum, part_dev);
  hipLaunchKernelGGL(coil_final_kernel, dim3(C), dim3(DP_THREADS), 0, st, part_sum, part_dev, G, n2, stats);
  return hipGetLastError();
}

}  // namespace inr
