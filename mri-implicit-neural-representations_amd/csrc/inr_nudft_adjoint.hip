// inr_nudft_adjoint.hip -- the conjugate transpose of inr_nudft (no reference counterpart): k-space
// samples at off-grid positions back onto the image grid.  val [C][M][2] fp32, pos [M][2] fp64 (u_y, u_x) in index units,
// w [M] fp32 or null (all ones) ->
//   out[c][y][x] = 1/sqrt(HW) sum_m w[m] val[c][m] exp(+2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
// c_y = H/2, c_x = W/2 (integer division).  inr_mi355x/trajectory.py::nudft_adjoint_numpy is the same text in fp64.
//
// Two launches on the caller's stream:
//   nudft_tables_kernel   (inr_nudft.hip) the forward call's phasor tables Ex[x][m], Ey[y][m] / sqrt(HW), sample index
//                         fastest, fp64 phase reduction, zero padding -- here with x padded to 64 like y, so that a tile
//                         reads them without a bounds check.  The contraction index m is the contiguous one of both.
//   adjoint_nudft_kernel  a workgroup (4 waves) owns 64 x 64 pixels (y, x) of one coil and walks m in chunks of 16 through
//                         LDS with the next chunk's global loads in flight:
//                           A[m][y] = conj(Ey[y][m]) (w[m] val[c][m])   one fp32 complex product, formed while staging
//                           B[m][x] = conj(Ex[x][m])
//                           out[y][x] = sum_m A[m][y] B[m][x]
//                         on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32, exact fp32, four real products per complex
//                         one).  Wave v holds rows 16 v .. 16 v + 15 of the tile, all 64 columns.
// val / w are read under m < M, out is written under y < H, x < W.  No atomics, a fixed order of additions: two calls give
// the same bits.  LDS rows are 80 floats, so the four k rows a wave reads at once lie 16 banks apart.
#include <hip/hip_runtime.h>
#include "inr_aux.h"

namespace inr {

namespace {

constexpr int AD_THREADS = 256;
constexpr int AD_T = 64;    // pixels per tile edge
constexpr int AD_TK = 16;   // samples per chunk
constexpr int AD_LD = 80;   // floats per LDS row
constexpr int AD_MPAD = 64; // the tables' padding of M (nudft_tables_kernel's)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AdjointDims {
  long long Mp;
  int Hp, Wp;
};

AdjointDims adjoint_dims(long long H, long long W, long long M) {
  AdjointDims d;
  d.Mp = (M + AD_MPAD - 1) / AD_MPAD * AD_MPAD;
  d.Hp = (int)((H + AD_T - 1) / AD_T * AD_T);
  d.Wp = (int)((W + AD_T - 1) / AD_T * AD_T);
  return d;
}

__global__ __launch_bounds__(AD_THREADS) void adjoint_nudft_kernel(const float* __restrict__ val,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ tab, const long long M,
                                                                    const long long Mp, const int H, const int W,
                                                                    const int Hp, const int Wp, float* __restrict__ out) {
  __shared__ float sAr[AD_TK * AD_LD], sAi[AD_TK * AD_LD], sBr[AD_TK * AD_LD], sBi[AD_TK * AD_LD];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l15 = lane & 15, lk = lane >> 4;
  const int tiles_x = Wp / AD_T;
  const int x0 = (int)(blockIdx.x % tiles_x) * AD_T, y0 = (int)(blockIdx.x / tiles_x) * AD_T, c = blockIdx.y;
  const float* exr = tab;
  const float* exi = exr + (size_t)Wp * Mp;
  const float* eyr = exi + (size_t)Wp * Mp;
  const float* eyi = eyr + (size_t)Hp * Mp;
  const float* valc = val + 2 * (size_t)c * M;
  // what this thread moves of a chunk: table row sn (of y and of x), samples sk..sk+3 of the chunk
  const int sn = t >> 2, sk = (t & 3) * 4;
  const size_t rowy = (size_t)(y0 + sn) * Mp, rowx = (size_t)(x0 + sn) * Mp;
  const long long nk = Mp / AD_TK;

  f32x4 accr[4], acci[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) accr[j] = acci[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 gyr, gyi, gxr, gxi;
  float2 gv[4];
  auto fetch = [&](long long kc) {
    const long long m = kc * AD_TK + sk;
    gyr = *reinterpret_cast<const float4*>(eyr + rowy + m);
    gyi = *reinterpret_cast<const float4*>(eyi + rowy + m);
    gxr = *reinterpret_cast<const float4*>(exr + rowx + m);
    gxi = *reinterpret_cast<const float4*>(exi + rowx + m);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float2 v = make_float2(0.f, 0.f);
      if (m + e < M) {
        v = *reinterpret_cast<const float2*>(valc + 2 * (m + e));
        if (w != nullptr) {
          const float we = w[m + e];
          v.x *= we;
          v.y *= we;
        }
      }
      gv[e] = v;
    }
  };
  fetch(0);
  for (long long kc = 0; kc < nk; ++kc) {
    __syncthreads();  // the previous chunk has been read
    {
      const float yr[4] = {gyr.x, gyr.y, gyr.z, gyr.w}, yi[4] = {gyi.x, gyi.y, gyi.z, gyi.w};
      const float xr[4] = {gxr.x, gxr.y, gxr.z, gxr.w}, xi[4] = {gxi.x, gxi.y, gxi.z, gxi.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // conj(Ey) v = (yr - i yi)(vr + i vi)
        sAr[(sk + e) * AD_LD + sn] = yr[e] * gv[e].x + yi[e] * gv[e].y;
        sAi[(sk + e) * AD_LD + sn] = yr[e] * gv[e].y - yi[e] * gv[e].x;
        sBr[(sk + e) * AD_LD + sn] = xr[e];
        sBi[(sk + e) * AD_LD + sn] = -xi[e];
      }
    }
    __syncthreads();
    if (kc + 1 < nk) fetch(kc + 1);
#pragma unroll
    for (int kk = 0; kk < AD_TK / 4; ++kk) {
      const int row = (4 * kk + lk) * AD_LD;
      const float ar = sAr[row + 16 * wave + l15], ai = sAi[row + 16 * wave + l15], nai = -ai;
      float br[4], bi[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        br[j] = sBr[row + 16 * j + l15];
        bi[j] = sBi[row + 16 * j + l15];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) accr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br[j], accr[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acci[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi[j], acci[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) accr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(nai, bi[j], accr[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acci[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br[j], acci[j], 0, 0, 0);
    }
  }
  // accumulator register r of block j is out[row y0 + 16 wave + 4 lk + r][column x0 + 16 j + l15]
  float* outc = out + 2 * (size_t)c * H * W;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int y = y0 + 16 * wave + 4 * lk + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + 16 * j + l15;
      if (y < H && x < W)
        *reinterpret_cast<float2*>(outc + 2 * ((size_t)y * W + x)) = make_float2(accr[j][r], acci[j][r]);
    }
  }
}

}  // namespace

long long adjoint_nudft_scratch_floats(long long H, long long W, long long M) {
  const AdjointDims d = adjoint_dims(H, W, M);
  return 2LL * ((long long)d.Wp + d.Hp) * d.Mp;
}

hipError_t launch_adjoint_nudft(const float* val, const double* pos, const float* w, int C, int H, int W, long long M,
                                float* out, float* scratch, hipStream_t st) {
  const AdjointDims d = adjoint_dims(H, W, M);
  launch_nudft_tables(pos, M, d.Mp, H, W, d.Hp, d.Wp, scratch, st);
  // H W < 2^31 (the entry's check) bounds the tile count by (H / 64 + 1)(W / 64 + 1) < 2^31
  const unsigned tiles = (unsigned)(d.Wp / AD_T) * (unsigned)(d.Hp / AD_T);
  hipLaunchKernelGGL(adjoint_nudft_kernel, dim3(tiles, (unsigned)C), dim3(AD_THREADS), 0, st, val, w, scratch, M, d.Mp,
                     H, W, d.Hp, d.Wp, out);
  return hipGetLastError();
}

}  // namespace inr
