// inr_nudft_adjoint.hip -- the conjugate transpose of inr_nudft (no reference counterpart): k-space
// samples at off-grid positions back onto the image grid.  val [C][M][2] fp32, pos [M][2] fp64 (u_y, u_x) in index units,
// w [M] fp32 or null (all ones) ->
//   out[c][y][x] = 1/sqrt(HW) sum_m w[m] val[c][m] exp(+2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
// c_y = H/2, c_x = W/2 (integer division).  inr_mi355x/trajectory.py::nudft_adjoint_numpy is the same text in fp64.
//
// Two launches on the caller's stream (tables, tile product and the determinism argument: inr_nudft_tile.h):
//   nudft_tables_kernel   (inr_nudft.hip) the forward call's tables, here with x padded to 64 like y.  The contraction
//                         index m is the contiguous one of both.
//   adjoint_nudft_kernel  a workgroup (4 waves) owns 64 x 64 pixels (y, x) of one coil and walks m in chunks of 16:
//                           A[m][y] = conj(Ey[y][m]) (w[m] val[c][m])   one fp32 complex product, formed while staging
//                           B[m][x] = conj(Ex[x][m])
//                           out[y][x] = sum_m A[m][y] B[m][x]           the tile product
// val / w are read under m < M, out is written under y < H, x < W.
#include <hip/hip_runtime.h>
#include "inr_aux.h"
#include "inr_nudft_tile.h"

namespace inr {

namespace {

// a tile is NT_TILE x NT_TILE pixels, a chunk NT_TK samples
__global__ __launch_bounds__(NT_THREADS) void adjoint_nudft_kernel(const float* __restrict__ val,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ tab, const long long M,
                                                                    const long long Mp, const int H, const int W,
                                                                    const int Hp, const int Wp, float* __restrict__ out) {
  __shared__ float sAr[NT_TK * NT_LD], sAi[NT_TK * NT_LD], sBr[NT_TK * NT_LD], sBi[NT_TK * NT_LD];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l15 = lane & 15, lk = lane >> 4;
  const int tiles_x = Wp / NT_TILE;
  const int x0 = (int)(blockIdx.x % tiles_x) * NT_TILE, y0 = (int)(blockIdx.x / tiles_x) * NT_TILE, c = blockIdx.y;
  const PhasorTables p = phasor_tables(tab, Mp, Hp, Wp);
  const float* valc = val + 2 * (size_t)c * M;
  // what this thread moves of a chunk: table row sn (of y and of x), samples sk..sk+3 of the chunk
  const int sn = t >> 2, sk = (t & 3) * 4;
  const size_t rowy = (size_t)(y0 + sn) * Mp, rowx = (size_t)(x0 + sn) * Mp;
  const long long nk = Mp / NT_TK;

  f32x4 accr[4], acci[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) accr[j] = acci[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 gyr, gyi, gxr, gxi;
  float2 gv[4];
  auto fetch = [&](long long kc) {
    const long long m = kc * NT_TK + sk;
    gyr = *reinterpret_cast<const float4*>(p.eyr + rowy + m);
    gyi = *reinterpret_cast<const float4*>(p.eyi + rowy + m);
    gxr = *reinterpret_cast<const float4*>(p.exr + rowx + m);
    gxi = *reinterpret_cast<const float4*>(p.exi + rowx + m);
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
        // conj(Ey) v = (yr - i yi)(vr + i vi): per part one rounded product and one fma, spelled out so that which of
        // the two products is rounded on its own is not the compiler's choice
        sAr[(sk + e) * NT_LD + sn] = __builtin_fmaf(yi[e], gv[e].y, yr[e] * gv[e].x);
        sAi[(sk + e) * NT_LD + sn] = __builtin_fmaf(-yi[e], gv[e].x, yr[e] * gv[e].y);
        sBr[(sk + e) * NT_LD + sn] = xr[e];
        sBi[(sk + e) * NT_LD + sn] = -xi[e];
      }
    }
    __syncthreads();
    if (kc + 1 < nk) fetch(kc + 1);
    cplx_tile_mma(sAr, sAi, sBr, sBi, wave, l15, lk, accr, acci);
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
  return phasor_floats(phasor_tables(H, W, M, NT_TILE, NT_TILE, nullptr));
}

hipError_t launch_adjoint_nudft(const float* val, const double* pos, const float* w, int C, int H, int W, long long M,
                                float* out, float* scratch, hipStream_t st) {
  const PhasorTables p = launch_nudft_tables(pos, M, H, W, NT_TILE, NT_TILE, scratch, st);
  // H W < 2^31 (the entry's check) bounds the tile count by (H / 64 + 1)(W / 64 + 1) < 2^31
  const unsigned tiles = (unsigned)(p.Wp / NT_TILE) * (unsigned)(p.Hp / NT_TILE);
  hipLaunchKernelGGL(adjoint_nudft_kernel, dim3(tiles, (unsigned)C), dim3(NT_THREADS), 0, st, val, w, scratch, M, p.Mp,
                     H, W, p.Hp, p.Wp, out);
  return hipGetLastError();
}

}  // namespace inr
