// bf16x3_probe.hip -- does v_mfma_f32_32x32x16_bf16 keep enough bits for an fp32 product rebuilt from bf16 pieces?
// An fp32 number is exactly hi + mid + lo with three bf16 terms (truncation split); six of the nine partial products
// (a1b1, a1b2, a2b1, a2b2, a1b3, a3b1) leave out terms <= 2^-24 |ab|.  What is not documented is how the instruction sums its
// 16 exact bf16 x bf16 products before the fp32 accumulate.  One wave forms a 32 x 32 x K product of random fp32 operands
//   v0: six products, a1b1 in one accumulator and the five corrections in a second one, added at the end
//   v1: six products into ONE accumulator
//   v2: a1b1 only (what plain bf16 truncation gives: the scale of the corrections)
//   v3: v_mfma_f32_32x32x2_f32 on the unsplit operands (the fp32 kernel's arithmetic)
// and the host prints each one's relative L2 error and its largest error over sum |a b| against float64, for operands
// uniform in [-1, 1) and for operands whose exponents spread over 2^+-6.
//   hipcc --offload-arch=gfx950 -O2 bf16x3_probe.hip -o bf16x3_probe && ./bf16x3_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int KMAX = 4096;

__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l) {
  h = __builtin_bit_cast(unsigned, x) & 0xffff0000u;
  const float r = x - __builtin_bit_cast(float, h);
  m = __builtin_bit_cast(unsigned, r) & 0xffff0000u;
  l = __builtin_bit_cast(unsigned, r - __builtin_bit_cast(float, m));
}

// 8 consecutive k of one row -> the three bf16 fragments
__device__ __forceinline__ void frag3(const float* p, bf16x8 (&f)[3]) {
  u32x4 o[3];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned h0, m0, l0, h1, m1, l1;
    split3(p[2 * e], h0, m0, l0);
    split3(p[2 * e + 1], h1, m1, l1);
    o[0][e] = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
    o[1][e] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
    o[2][e] = __builtin_amdgcn_perm(l1, l0, 0x07060302u);
  }
#pragma unroll
  for (int p3 = 0; p3 < 3; ++p3) f[p3] = __builtin_bit_cast(bf16x8, o[p3]);
}

// A, B: [32][K] row-major (K-contiguous, as the weight-gradient GEMM's operands); out: [4 variants][32][32]
__global__ __launch_bounds__(64) void probe(const float* A, const float* B, float* out, int K) {
  const int lane = threadIdx.x, li = lane & 31, half = lane >> 5;
  f32x16 c0, c1, s1, t1, f1;
#pragma unroll
  for (int r = 0; r < 16; ++r) c0[r] = c1[r] = s1[r] = t1[r] = f1[r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    bf16x8 a[3], b[3];
    frag3(A + li * K + k0 + 8 * half, a);
    frag3(B + li * K + k0 + 8 * half, b);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c1, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c1, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c1, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c1, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c1, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], s1, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], s1, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], s1, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], s1, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], s1, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], s1, 0, 0, 0);
    t1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], t1, 0, 0, 0);
    // fp32: lane (li, half) supplies k = half of each K = 2 step
#pragma unroll
    for (int e = 0; e < 8; ++e)
      f1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A[li * K + k0 + 2 * e + half], B[li * K + k0 + 2 * e + half], f1, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    out[0 * 1024 + row * 32 + li] = c0[r] + c1[r];
    out[1 * 1024 + row * 32 + li] = s1[r];
    out[2 * 1024 + row * 32 + li] = t1[r];
    out[3 * 1024 + row * 32 + li] = f1[r];
  }
}

static float rnd() { return (float)(rand() / (RAND_MAX + 1.0) * 2.0 - 1.0); }

int main() {
  float *dA, *dB, *dO;
  hipMalloc(&dA, 32 * KMAX * sizeof(float));
  hipMalloc(&dB, 32 * KMAX * sizeof(float));
  hipMalloc(&dO, 4 * 1024 * sizeof(float));
  const char* names[4] = {"six products, two accumulators", "six products, one accumulator", "a1 b1 only",
                          "fp32 MFMA 32x32x2"};
  srand(3);
  for (int spread = 0; spread < 2; ++spread)
    for (int K : {16, 512, 4096}) {
      std::vector<float> A(32 * K), B(32 * K), O(4 * 1024);
      for (auto& x : A) x = rnd() * (spread ? std::ldexp(1.f, rand() % 13 - 6) : 1.f);
      for (auto& x : B) x = rnd() * (spread ? std::ldexp(1.f, rand() % 13 - 6) : 1.f);
      hipMemcpy(dA, A.data(), A.size() * sizeof(float), hipMemcpyHostToDevice);
      hipMemcpy(dB, B.data(), B.size() * sizeof(float), hipMemcpyHostToDevice);
      hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dO, K);
      if (hipMemcpy(O.data(), dO, O.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
      printf("K = %d, %s operands\n", K, spread ? "exponents over 2^+-6," : "uniform");
      for (int v = 0; v < 4; ++v) {
        double num = 0, den = 0, worst = 0;
        for (int m = 0; m < 32; ++m)
          for (int n = 0; n < 32; ++n) {
            double ref = 0, mag = 0;
            for (int k = 0; k < K; ++k) ref += (double)A[m * K + k] * B[n * K + k], mag += std::fabs((double)A[m * K + k] * B[n * K + k]);
            const double d = (double)O[v * 1024 + m * 32 + n] - ref;
            num += d * d, den += ref * ref;
            worst = std::fmax(worst, std::fabs(d) / mag);
          }
        printf("  %-32s rel L2 %.3e   max |err| / sum|ab| %.3e\n", names[v], std::sqrt(num / den), worst);
      }
    }
  return 0;
}
