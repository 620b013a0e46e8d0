// inr_nudft.hip -- the continuous k-space of coil images at off-grid positions (no reference
// counterpart).  img [C][H][W][2] fp32, pos [M][2] fp64 (u_y, u_x) in index units ->
//   out[c][m] = 1/sqrt(HW) sum_y sum_x I_c[y][x] exp(-2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
// c_y = H/2, c_x = W/2 (integer division).  inr_mi355x/trajectory.py::nudft_numpy is the same text in fp64.
//
// Two launches on the caller's stream:
//   nudft_tables_kernel  phasor tables in the caller's scratch, sample index fastest, planar re / im:
//                          Ex[x][m] = exp(-2 pi i frac((u_x - c_x)(x - c_x)/W)),  Ey[y][m] = the same in y, times 1/sqrt(HW).
//                        The phase is reduced in fp64 (t - rint(t)), sincospi is fp64, and each entry is rounded to
//                        fp32 once.  m is padded to a multiple of 64, x to 16 and y to 64, all padding is zero, so the
//                        contraction reads the tables without a bounds check.
//   nudft_kernel         a workgroup (4 waves) owns 64 samples of one coil.  For each tile of 64 image rows it forms
//                          T[m][y] = sum_x Ex[x][m] I[y][x]
//                        on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32, exact fp32, four real products per complex
//                        one), x in chunks of 16 through LDS with the next chunk's global loads in flight, then adds
//                        Ey[y][m] T[m][y] into 4 complex accumulators per lane: T never exists in memory.  The 16
//                        lanes that share a sample are added in lane order through LDS at the end.
// No atomics, a fixed order of additions: two calls give the same bits.  LDS rows are 80 floats, so the four k rows a
// wave reads at once lie 16 banks apart.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

namespace inr {

namespace {

constexpr int NU_THREADS = 256;
constexpr int NU_TM = NUDFT_TILE;  // samples per workgroup
constexpr int NU_TN = 64;          // image rows per tile
constexpr int NU_TK = 16;          // image columns per chunk
constexpr int NU_LD = 80;          // floats per LDS row
static_assert(NU_TM == 64 && NU_THREADS == 256, "the lane maps below are written for 4 waves x 16 samples");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct NudftDims {
  long long Mp;  // M rounded up to NU_TM
  int Hp, Wp;    // H rounded up to NU_TN, W to NU_TK
};

NudftDims nudft_dims(long long H, long long W, long long M) {
  NudftDims d;
  d.Mp = (M + NU_TM - 1) / NU_TM * NU_TM;
  d.Hp = (int)((H + NU_TN - 1) / NU_TN * NU_TN);
  d.Wp = (int)((W + NU_TK - 1) / NU_TK * NU_TK);
  return d;
}

// tab: ExR [Wp][Mp], ExI [Wp][Mp], EyR [Hp][Mp], EyI [Hp][Mp]
__global__ __launch_bounds__(NU_THREADS) void nudft_tables_kernel(const double* __restrict__ pos, const long long M,
                                                                   const long long Mp, const int H, const int W,
                                                                   const int Hp, const int Wp, float* __restrict__ tab) {
  const long long m = (long long)blockIdx.x * NU_THREADS + threadIdx.x;
  if (m >= Mp) return;
  const bool live = m < M;
  double uy = 0.0, ux = 0.0;
  if (live) {
    uy = pos[2 * m];
    ux = pos[2 * m + 1];
  }
  const double scale = 1.0 / sqrt((double)H * (double)W);
  float* exr = tab;
  float* exi = exr + (size_t)Wp * Mp;
  float* eyr = exi + (size_t)Wp * Mp;
  float* eyi = eyr + (size_t)Hp * Mp;
  for (int j = blockIdx.y; j < Wp + Hp; j += gridDim.y) {
    const bool isx = j < Wp;
    const int jj = isx ? j : j - Wp;
    const int n = isx ? W : H;
    float re = 0.f, im = 0.f;
    if (live && jj < n) {
      const int c = n / 2;
      double t = ((isx ? ux : uy) - (double)c) * (double)(jj - c) / (double)n;
      t -= rint(t);
      double s, co;
      sincospi(2.0 * t, &s, &co);
      const double k = isx ? 1.0 : scale;
      re = (float)(co * k);
      im = (float)(-s * k);
    }
    const size_t at = (size_t)jj * Mp + m;
    (isx ? exr : eyr)[at] = re;
    (isx ? exi : eyi)[at] = im;
  }
}

__global__ __launch_bounds__(NU_THREADS) void nudft_kernel(const float* __restrict__ img, const float* __restrict__ tab,
                                                            const long long M, const long long Mp, const int H,
                                                            const int W, const int Hp, const int Wp,
                                                            float* __restrict__ out) {
  __shared__ float sAr[NU_TK * NU_LD], sAi[NU_TK * NU_LD], sBr[NU_TK * NU_LD], sBi[NU_TK * NU_LD];
  __shared__ float red[2][NU_TM][17];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l15 = lane & 15, lk = lane >> 4;
  const size_t m0 = (size_t)blockIdx.x * NU_TM;
  const int c = blockIdx.y;
  const float* exr = tab;
  const float* exi = exr + (size_t)Wp * Mp;
  const float* eyr = exi + (size_t)Wp * Mp;
  const float* eyi = eyr + (size_t)Hp * Mp;
  const float* imgc = img + 2 * (size_t)c * H * W;
  // what this thread moves of a chunk: Ex rows ak, samples am..am+3; image row bn, columns bk..bk+3
  const int ak = t >> 4, am = (t & 15) * 4;
  const int bn = t >> 2, bk = (t & 3) * 4;
  const int nk = Wp / NU_TK;

  float accr[4] = {0.f, 0.f, 0.f, 0.f}, acci[4] = {0.f, 0.f, 0.f, 0.f};
  for (int y0 = 0; y0 < Hp; y0 += NU_TN) {
    f32x4 tr[4], ti[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tr[j] = ti[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 gar, gai;
    float2 gb[4];
    const int y = y0 + bn;
    auto fetch = [&](int kc) {
      const size_t a = (size_t)(kc * NU_TK + ak) * Mp + m0 + am;
      gar = *reinterpret_cast<const float4*>(exr + a);
      gai = *reinterpret_cast<const float4*>(exi + a);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = kc * NU_TK + bk + e;
        gb[e] = (y < H && x < W) ? *reinterpret_cast<const float2*>(imgc + 2 * ((size_t)y * W + x)) : make_float2(0.f, 0.f);
      }
    };
    fetch(0);
    for (int kc = 0; kc < nk; ++kc) {
      __syncthreads();  // the previous chunk has been read
      *reinterpret_cast<float4*>(sAr + ak * NU_LD + am) = gar;
      *reinterpret_cast<float4*>(sAi + ak * NU_LD + am) = gai;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sBr[(bk + e) * NU_LD + bn] = gb[e].x;
        sBi[(bk + e) * NU_LD + bn] = gb[e].y;
      }
      __syncthreads();
      if (kc + 1 < nk) fetch(kc + 1);
#pragma unroll
      for (int kk = 0; kk < NU_TK / 4; ++kk) {
        const int row = (4 * kk + lk) * NU_LD;
        const float ar = sAr[row + 16 * wave + l15], ai = sAi[row + 16 * wave + l15], nai = -ai;
        float br[4], bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          br[j] = sBr[row + 16 * j + l15];
          bi[j] = sBi[row + 16 * j + l15];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) tr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br[j], tr[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) ti[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi[j], ti[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) tr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(nai, bi[j], tr[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) ti[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br[j], ti[j], 0, 0, 0);
      }
    }
    // accumulator register r of block j is T[sample 16 wave + 4 lk + r][row y0 + 16 j + l15]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t e = (size_t)(y0 + 16 * j + l15) * Mp + m0 + 16 * wave + 4 * lk;
      const float4 er = *reinterpret_cast<const float4*>(eyr + e);
      const float4 ei = *reinterpret_cast<const float4*>(eyi + e);
      const float err[4] = {er.x, er.y, er.z, er.w}, eii[4] = {ei.x, ei.y, ei.z, ei.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        accr[r] += err[r] * tr[j][r] - eii[r] * ti[j][r];
        acci[r] += err[r] * ti[j][r] + eii[r] * tr[j][r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[0][16 * wave + 4 * lk + r][l15] = accr[r];
    red[1][16 * wave + 4 * lk + r][l15] = acci[r];
  }
  __syncthreads();
  if (t < NU_TM && m0 + t < (size_t)M) {
    float re = red[0][t][0], im = red[1][t][0];
    for (int u = 1; u < 16; ++u) {
      re += red[0][t][u];
      im += red[1][t][u];
    }
    *reinterpret_cast<float2*>(out + 2 * ((size_t)c * M + m0 + t)) = make_float2(re, im);
  }
}

}  // namespace

long long nudft_scratch_floats(long long H, long long W, long long M) {
  const NudftDims d = nudft_dims(H, W, M);
  return 2LL * ((long long)d.Wp + d.Hp) * d.Mp;
}

void launch_nudft_tables(const double* pos, long long M, long long Mp, int H, int W, int Hp, int Wp, float* tab,
                         hipStream_t st) {
  const int rows = Wp + Hp;
  const dim3 tgrid((unsigned)((Mp + NU_THREADS - 1) / NU_THREADS), (unsigned)(rows < 65535 ? rows : 65535));
  hipLaunchKernelGGL(nudft_tables_kernel, tgrid, dim3(NU_THREADS), 0, st, pos, M, Mp, H, W, Hp, Wp, tab);
}

hipError_t launch_nudft(const float* img, int C, int H, int W, const double* pos, long long M, float* out,
                        float* scratch, hipStream_t st) {
  const NudftDims d = nudft_dims(H, W, M);
  launch_nudft_tables(pos, M, d.Mp, H, W, d.Hp, d.Wp, scratch, st);
  hipLaunchKernelGGL(nudft_kernel, dim3((unsigned)(d.Mp / NU_TM), (unsigned)C), dim3(NU_THREADS), 0, st, img, scratch, M,
                     d.Mp, H, W, d.Hp, d.Wp, out);
  return hipGetLastError();
}

}  // namespace inr
