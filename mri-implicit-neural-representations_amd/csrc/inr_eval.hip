// inr_eval.hip -- image metrics of the validation epoch (train.py:221-231; models/utils.py:227-250) on gfx950:
// root-sum-of-squares over coils, PSNR and SSIM against a ground-truth RSS image.  Three launches, no atomics, no
// host synchronisation; every reduction runs in a fixed order, so results are bitwise reproducible.
//
//   pass 1  one pixel per lane (grid-stride over H*W): |z| per coil, RSS in fixed coil order (fp32, no contraction,
//           as fastmri.complex_abs + rss evaluate it), and per-block partials of the squared error (fp64) and of the
//           extrema of both images;
//   pass 2  2-D tiles of 32 x 16 interior pixels with a 3-pixel halo in LDS: horizontal then vertical 7-sums of
//           x, y, x^2, y^2, xy in fp64, S per interior pixel, one fp64 partial per block.  Every block first folds
//           pass 1's extrema (exact in any order) into the data range R;
//   final   one block: fixed-order sums of the partials -> [psnr, ssim, sse, max_ref, min_ref, max_rec, min_rec, R].
//
// SSIM is skimage.metrics.structural_similarity(x, x_hat, data_range=R) of scikit-image 0.18.1: inputs cast to
// float64, 7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance (49 / 48), mean over the interior cropped by
// 3 pixels (so uniform_filter's boundary mode never enters).  R = max(max x, max x_hat) - min(min x, min x_hat) in
// float32, as numpy evaluates it on float32 arrays; R = 0 gives NaN as there.
#include <hip/hip_runtime.h>
#include <cmath>
#include "inr_aux.h"
#include "inr_reduce.h"

namespace inr {

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_P1_MAX_BLOCKS = 512;
constexpr int EV_TW = 32, EV_TH = 16, EV_HALO = 3;
constexpr int EV_LW = EV_TW + 2 * EV_HALO, EV_LH = EV_TH + 2 * EV_HALO;

inline int p1_blocks(long long n) {
  const long long b = (n + EV_THREADS - 1) / EV_THREADS;
  return (int)(b < EV_P1_MAX_BLOCKS ? b : EV_P1_MAX_BLOCKS);
}
inline int p2_gx(long long W) { return (int)((W - 2 * EV_HALO + EV_TW - 1) / EV_TW); }
inline int p2_gy(long long H) { return (int)((H - 2 * EV_HALO + EV_TH - 1) / EV_TH); }

// part1 layout: [5][G1] doubles = sse, max_ref, min_ref, max_rec, min_rec of each pass-1 block
__global__ __launch_bounds__(EV_THREADS) void eval_rss_kernel(const float2* __restrict__ coils, int C, long long n,
                                                               const float* __restrict__ ref, float* __restrict__ rss,
                                                               double* __restrict__ part1) {
  __shared__ double dred[EV_THREADS];
  __shared__ float fred[EV_THREADS];
  double sse = 0.0;
  float mxr = -INFINITY, mnr = INFINITY, mxx = -INFINITY, mnx = INFINITY;
  const long long stride = (long long)gridDim.x * EV_THREADS;
  for (long long p = (long long)blockIdx.x * EV_THREADS + threadIdx.x; p < n; p += stride) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float2 z = coils[(long long)c * n + p];
      const float m = __fsqrt_rn(__fadd_rn(__fmul_rn(z.x, z.x), __fmul_rn(z.y, z.y)));  // complex_abs
      s = __fadd_rn(s, __fmul_rn(m, m));                                                 // rss: sum_c |z|^2
    }
    const float r = __fsqrt_rn(s);
    rss[p] = r;
    mxr = fmaxf(mxr, r);
    mnr = fminf(mnr, r);
    if (ref != nullptr) {
      const float x = ref[p];
      const float d = __fsub_rn(x, r);
      sse += (double)d * (double)d;
      mxx = fmaxf(mxx, x);
      mnx = fminf(mnx, x);
    }
  }
  if (part1 == nullptr) return;  // RSS only (uniform over the grid: no lane leaves a barrier below)
  const int G = gridDim.x, b = blockIdx.x;
  sse = block_reduce<EV_THREADS>(sse, dred, Sum());
  mxx = block_reduce<EV_THREADS>(mxx, fred, MaxF());
  mnx = block_reduce<EV_THREADS>(mnx, fred, MinF());
  mxr = block_reduce<EV_THREADS>(mxr, fred, MaxF());
  mnr = block_reduce<EV_THREADS>(mnr, fred, MinF());
  if (threadIdx.x == 0) {
    part1[0 * G + b] = sse;
    part1[1 * G + b] = mxx;
    part1[2 * G + b] = mnx;
    part1[3 * G + b] = mxr;
    part1[4 * G + b] = mnr;
  }
}

// extrema of pass 1 (max_ref, min_ref, max_rec, min_rec), the same in every block
__device__ void fold_extrema(const double* __restrict__ part1, int G1, float* fred, float ext[4]) {
  float a = -INFINITY, b = INFINITY, c = -INFINITY, d = INFINITY;
  for (int i = threadIdx.x; i < G1; i += EV_THREADS) {
    a = fmaxf(a, (float)part1[1 * G1 + i]);
    b = fminf(b, (float)part1[2 * G1 + i]);
    c = fmaxf(c, (float)part1[3 * G1 + i]);
    d = fminf(d, (float)part1[4 * G1 + i]);
  }
  ext[0] = block_reduce<EV_THREADS>(a, fred, MaxF());
  ext[1] = block_reduce<EV_THREADS>(b, fred, MinF());
  ext[2] = block_reduce<EV_THREADS>(c, fred, MaxF());
  ext[3] = block_reduce<EV_THREADS>(d, fred, MinF());
}

// np.maximum(x.max(), xhat.max()) - np.minimum(x.min(), xhat.min()) on float32 scalars
__device__ float data_range(const float ext[4]) {
  return __fsub_rn(fmaxf(ext[0], ext[2]), fminf(ext[1], ext[3]));
}

__global__ __launch_bounds__(EV_THREADS) void eval_ssim_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                                int H, int W, const double* __restrict__ part1, int G1,
                                                                double* __restrict__ part2) {
  __shared__ float sx[EV_LH][EV_LW], sy[EV_LH][EV_LW];
  __shared__ double hs[5][EV_LH][EV_TW];
  __shared__ double dred[EV_THREADS];
  __shared__ float fred[EV_THREADS];
  const int tid = threadIdx.x;
  float ext[4];
  fold_extrema(part1, G1, fred, ext);
  const double R = (double)data_range(ext);
  const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);

  // tile: interior rows [i0 + 3, i0 + 3 + TH), columns [j0 + 3, j0 + 3 + TW); loaded rows [i0, i0 + LH) (zero past the edge)
  const int i0 = blockIdx.y * EV_TH, j0 = blockIdx.x * EV_TW;
  for (int k = tid; k < EV_LH * EV_LW; k += EV_THREADS) {
    const int r = k / EV_LW, c = k - r * EV_LW;
    const int gi = i0 + r, gj = j0 + c;
    const bool in = gi < H && gj < W;
    const long long off = (long long)gi * W + gj;
    sx[r][c] = in ? xs[off] : 0.f;
    sy[r][c] = in ? ys[off] : 0.f;
  }
  __syncthreads();
  // horizontal 7-sums of x, y, x^2, y^2, xy (fp64: float * float is exact in double)
  for (int k = tid; k < EV_LH * EV_TW; k += EV_THREADS) {
    const int r = k / EV_TW, c = k - r * EV_TW;
    double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      const double x = sx[r][c + t], y = sy[r][c + t];
      a += x;
      b += y;
      aa += x * x;
      bb += y * y;
      ab += x * y;
    }
    hs[0][r][c] = a;
    hs[1][r][c] = b;
    hs[2][r][c] = aa;
    hs[3][r][c] = bb;
    hs[4][r][c] = ab;
  }
  __syncthreads();
  // vertical 7-sums and S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
  const double inv_np = 1.0 / 49.0, cov_norm = 49.0 / 48.0;
  const int c = tid % EV_TW;
  double acc = 0.0;
  for (int r = tid / EV_TW; r < EV_TH; r += EV_THREADS / EV_TW) {
    const int gi = i0 + r + EV_HALO, gj = j0 + c + EV_HALO;
    if (gi >= H - EV_HALO || gj >= W - EV_HALO) continue;
    double s[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double v = 0.0;
#pragma unroll
      for (int t = 0; t < 7; ++t) v += hs[q][r + t][c];
      s[q] = v * inv_np;
    }
    const double ux = s[0], uy = s[1];
    const double vx = cov_norm * (s[2] - ux * ux);
    const double vy = cov_norm * (s[3] - uy * uy);
    const double vxy = cov_norm * (s[4] - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
    const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    acc += (A1 * A2) / (B1 * B2);
  }
  acc = block_reduce<EV_THREADS>(acc, dred, Sum());
  if (tid == 0) part2[blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// out: psnr, ssim, sse, max_ref, min_ref, max_rec, min_rec, data_range
__global__ __launch_bounds__(EV_THREADS) void eval_finalize_kernel(const double* __restrict__ part1, int G1,
                                                                    const double* __restrict__ part2, int G2, int H, int W,
                                                                    double* __restrict__ out) {
  __shared__ double dred[EV_THREADS];
  __shared__ float fred[EV_THREADS];
  double sse = 0.0, ss = 0.0;
  for (int i = threadIdx.x; i < G1; i += EV_THREADS) sse += part1[i];
  for (int i = threadIdx.x; i < G2; i += EV_THREADS) ss += part2[i];
  sse = block_reduce<EV_THREADS>(sse, dred, Sum());
  ss = block_reduce<EV_THREADS>(ss, dred, Sum());
  float ext[4];
  fold_extrema(part1, G1, fred, ext);
  if (threadIdx.x == 0) {
    const float R = data_range(ext);
    const double n = (double)H * (double)W;
    const double interior = (double)(H - 2 * EV_HALO) * (double)(W - 2 * EV_HALO);
    out[0] = 10.0 * log10((double)ext[0] / (sse / n + 1e-10));  // models/utils.py:248: max(x), not max(x)^2
    out[1] = R == 0.f ? (double)NAN : ss / interior;
    out[2] = sse;
    out[3] = ext[0];
    out[4] = ext[1];
    out[5] = ext[2];
    out[6] = ext[3];
    out[7] = R;
  }
}

}  // namespace

long long image_metrics_scratch_doubles(long long H, long long W) {
  long long s = 5LL * p1_blocks(H * W);
  if (H >= 7 && W >= 7) s += (long long)p2_gx(W) * p2_gy(H);
  return s;
}

hipError_t launch_image_metrics(const float* coils, int C, int H, int W, const float* ref, float* rss_out,
                                double* metrics_out, double* scratch, hipStream_t st) {
  const long long n = (long long)H * W;
  const int G1 = p1_blocks(n);
  double* part1 = ref != nullptr ? scratch : nullptr;
  hipLaunchKernelGGL(eval_rss_kernel, dim3(G1), dim3(EV_THREADS), 0, st, reinterpret_cast<const float2*>(coils), C, n,
                     ref, rss_out, part1);
  if (ref == nullptr) return hipGetLastError();
  const int gx = p2_gx(W), gy = p2_gy(H);
  double* part2 = scratch + 5LL * G1;
  hipLaunchKernelGGL(eval_ssim_kernel, dim3(gx, gy), dim3(EV_THREADS), 0, st, ref, rss_out, H, W, part1, G1, part2);
  hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(EV_THREADS), 0, st, part1, G1, part2, gx * gy, H, W,
                     metrics_out);
  return hipGetLastError();
}

}  // namespace inr
