// inr_nudft_tile.h -- what inr_nudft.hip and inr_nudft_adjoint.hip share: the phasor tables and the
// complex 64 x 64 x 16 tile product.
//
// The tables (nudft_tables_kernel, inr_nudft.hip) lie in the caller's scratch, sample index fastest, planar re / im:
//   Ex[x][m] = exp(-2 pi i frac((u_x - c_x)(x - c_x)/W)),  Ey[y][m] = the same in y, times 1/sqrt(HW).
// The phase is reduced in fp64 (t - rint(t)), sincospi is fp64, and each entry is rounded to fp32 once.  m is padded to a
// multiple of 64, y and x to what the reading kernel's tile asks for; all padding is zero, so a contraction reads the
// tables without a bounds check.
//
// The product runs on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32, exact fp32, four real products per complex one), its
// contraction index in chunks of 16 through LDS with the next chunk's global loads in flight.  No atomics, a fixed order
// of additions: two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace inr {

constexpr int NT_THREADS = 256;  // 4 waves
constexpr int NT_TILE = 64;      // tile edge: wave v owns rows 16 v .. 16 v + 15 of A, all 64 columns of B
constexpr int NT_TK = 16;        // contraction entries per chunk
constexpr int NT_LD = 80;        // floats per LDS row: the four k rows a wave reads at once lie 16 banks apart
constexpr int NT_MPAD = 64;      // the tables' padding of M
static_assert(NT_TILE == 64 && NT_THREADS == 256, "the lane maps are written for 4 waves x 16");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ExR [Wp][Mp], ExI [Wp][Mp], EyR [Hp][Mp], EyI [Hp][Mp], one behind the other
struct PhasorTables {
  const float *exr, *exi, *eyr, *eyi;
  long long Mp;
  int Hp, Wp;
};

__host__ __device__ inline PhasorTables phasor_tables(const float* tab, long long Mp, int Hp, int Wp) {
  PhasorTables p;
  p.exr = tab;
  p.exi = p.exr + (size_t)Wp * Mp;
  p.eyr = p.exi + (size_t)Wp * Mp;
  p.eyi = p.eyr + (size_t)Hp * Mp;
  p.Mp = Mp;
  p.Hp = Hp;
  p.Wp = Wp;
  return p;
}

// the tables of M samples of an H x W image, H padded to a multiple of pad_h and W of pad_w
inline PhasorTables phasor_tables(long long H, long long W, long long M, int pad_h, int pad_w, const float* scratch) {
  return phasor_tables(scratch, (M + NT_MPAD - 1) / NT_MPAD * NT_MPAD, (int)((H + pad_h - 1) / pad_h * pad_h),
                       (int)((W + pad_w - 1) / pad_w * pad_w));
}

inline long long phasor_floats(const PhasorTables& p) { return 2LL * ((long long)p.Wp + p.Hp) * p.Mp; }

// fills the tables of those sizes in `scratch` (inr_nudft.hip) and returns their description
PhasorTables launch_nudft_tables(const double* pos, long long M, int H, int W, int pad_h, int pad_w, float* scratch,
                                 hipStream_t st);

// One staged chunk: acc += A^T B for A [NT_TK][64] (re sAr, im sAi) and B [NT_TK][64] (sBr, sBi), rows of NT_LD floats.
// Register r of acc_*[j] is the entry (16 wave + 4 lk + r, 16 j + l15).
__device__ __forceinline__ void cplx_tile_mma(const float* sAr, const float* sAi, const float* sBr, const float* sBi,
                                              const int wave, const int l15, const int lk, f32x4 (&acc_re)[4],
                                              f32x4 (&acc_im)[4]) {
#pragma unroll
  for (int kk = 0; kk < NT_TK / 4; ++kk) {
    const int row = (4 * kk + lk) * NT_LD;
    const float ar = sAr[row + 16 * wave + l15], ai = sAi[row + 16 * wave + l15], nai = -ai;
    float br[4], bi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      br[j] = sBr[row + 16 * j + l15];
      bi[j] = sBi[row + 16 * j + l15];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc_re[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br[j], acc_re[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc_im[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi[j], acc_im[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc_re[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(nai, bi[j], acc_re[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc_im[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br[j], acc_im[j], 0, 0, 0);
  }
}

}  // namespace inr
