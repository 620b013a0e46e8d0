// inr_nudft.hip -- the continuous k-space of coil images at off-grid positions (no reference
// counterpart).  img [C][H][W][2] fp32, pos [M][2] fp64 (u_y, u_x) in index units ->
//   out[c][m] = 1/sqrt(HW) sum_y sum_x I_c[y][x] exp(-2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
// c_y = H/2, c_x = W/2 (integer division).  inr_mi355x/trajectory.py::nudft_numpy is the same text in fp64.
//
// Two launches on the caller's stream (tables, tile product and the determinism argument: inr_nudft_tile.h):
//   nudft_tables_kernel  the phasor tables Ex[x][m], Ey[y][m] / sqrt(HW) in the caller's scratch, here with x padded to
//                        16 and y to 64.
//   nudft_kernel         a workgroup (4 waves) owns 64 samples of one coil.  For each tile of 64 image rows it forms
//                          T[m][y] = sum_x Ex[x][m] I[y][x]
//                        by the tile product, x in chunks of 16, then adds Ey[y][m] T[m][y] into 4 complex accumulators
//                        per lane: T never exists in memory.  The 16 lanes that share a sample are added in lane order
//                        through LDS at the end.
#include <hip/hip_runtime.h>
#include "inr_aux.h"
#include "inr_nudft_tile.h"

namespace inr {

namespace {

// a workgroup's NT_TILE samples meet NT_TILE image rows per tile, NT_TK image columns per chunk
static_assert(NT_TILE == NUDFT_TILE, "inr_aux.h and inr_nudft_tile.h disagree");

__global__ __launch_bounds__(NT_THREADS) void nudft_tables_kernel(const double* __restrict__ pos, const long long M,
                                                                   const long long Mp, const int H, const int W,
                                                                   const int Hp, const int Wp, float* __restrict__ tab) {
  const long long m = (long long)blockIdx.x * NT_THREADS + threadIdx.x;
  if (m >= Mp) return;
  const bool live = m < M;
  double uy = 0.0, ux = 0.0;
  if (live) {
    uy = pos[2 * m];
    ux = pos[2 * m + 1];
  }
  const double scale = 1.0 / sqrt((double)H * (double)W);
  const PhasorTables p = phasor_tables(tab, Mp, Hp, Wp);
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
    tab[(isx ? p.exr : p.eyr) - tab + at] = re;
    tab[(isx ? p.exi : p.eyi) - tab + at] = im;
  }
}

__global__ __launch_bounds__(NT_THREADS) void nudft_kernel(const float* __restrict__ img, const float* __restrict__ tab,
                                                            const long long M, const long long Mp, const int H,
                                                            const int W, const int Hp, const int Wp,
                                                            float* __restrict__ out) {
  __shared__ float sAr[NT_TK * NT_LD], sAi[NT_TK * NT_LD], sBr[NT_TK * NT_LD], sBi[NT_TK * NT_LD];
  __shared__ float red[2][NT_TILE][17];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l15 = lane & 15, lk = lane >> 4;
  const size_t m0 = (size_t)blockIdx.x * NT_TILE;
  const int c = blockIdx.y;
  const PhasorTables p = phasor_tables(tab, Mp, Hp, Wp);
  const float* imgc = img + 2 * (size_t)c * H * W;
  // what this thread moves of a chunk: Ex rows ak, samples am..am+3; image row bn, columns bk..bk+3
  const int ak = t >> 4, am = (t & 15) * 4;
  const int bn = t >> 2, bk = (t & 3) * 4;
  const int nk = Wp / NT_TK;

  float accr[4] = {0.f, 0.f, 0.f, 0.f}, acci[4] = {0.f, 0.f, 0.f, 0.f};
  for (int y0 = 0; y0 < Hp; y0 += NT_TILE) {
    f32x4 tr[4], ti[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tr[j] = ti[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 gar, gai;
    float2 gb[4];
    const int y = y0 + bn;
    auto fetch = [&](int kc) {
      const size_t a = (size_t)(kc * NT_TK + ak) * Mp + m0 + am;
      gar = *reinterpret_cast<const float4*>(p.exr + a);
      gai = *reinterpret_cast<const float4*>(p.exi + a);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = kc * NT_TK + bk + e;
        gb[e] = (y < H && x < W) ? *reinterpret_cast<const float2*>(imgc + 2 * ((size_t)y * W + x)) : make_float2(0.f, 0.f);
      }
    };
    fetch(0);
    for (int kc = 0; kc < nk; ++kc) {
      __syncthreads();  // the previous chunk has been read
      *reinterpret_cast<float4*>(sAr + ak * NT_LD + am) = gar;
      *reinterpret_cast<float4*>(sAi + ak * NT_LD + am) = gai;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sBr[(bk + e) * NT_LD + bn] = gb[e].x;
        sBi[(bk + e) * NT_LD + bn] = gb[e].y;
      }
      __syncthreads();
      if (kc + 1 < nk) fetch(kc + 1);
      cplx_tile_mma(sAr, sAi, sBr, sBi, wave, l15, lk, tr, ti);
    }
    // accumulator register r of block j is T[sample 16 wave + 4 lk + r][row y0 + 16 j + l15]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t e = (size_t)(y0 + 16 * j + l15) * Mp + m0 + 16 * wave + 4 * lk;
      const float4 er = *reinterpret_cast<const float4*>(p.eyr + e);
      const float4 ei = *reinterpret_cast<const float4*>(p.eyi + e);
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
  if (t < NT_TILE && m0 + t < (size_t)M) {
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
  return phasor_floats(phasor_tables(H, W, M, NT_TILE, NT_TK, nullptr));
}

PhasorTables launch_nudft_tables(const double* pos, long long M, int H, int W, int pad_h, int pad_w, float* scratch,
                                 hipStream_t st) {
  const PhasorTables p = phasor_tables(H, W, M, pad_h, pad_w, scratch);
  const int rows = p.Wp + p.Hp;
  const dim3 tgrid((unsigned)((p.Mp + NT_THREADS - 1) / NT_THREADS), (unsigned)(rows < 65535 ? rows : 65535));
  hipLaunchKernelGGL(nudft_tables_kernel, tgrid, dim3(NT_THREADS), 0, st, pos, M, p.Mp, H, W, p.Hp, p.Wp, scratch);
  return p;
}

hipError_t launch_nudft(const float* img, int C, int H, int W, const double* pos, long long M, float* out,
                        float* scratch, hipStream_t st) {
  const PhasorTables p = launch_nudft_tables(pos, M, H, W, NT_TILE, NT_TK, scratch, st);
  hipLaunchKernelGGL(nudft_kernel, dim3((unsigned)(p.Mp / NT_TILE), (unsigned)C), dim3(NT_THREADS), 0, st, img, scratch,
                     M, p.Mp, H, W, p.Hp, p.Wp, out);
  return hipGetLastError();
}

}  // namespace inr
