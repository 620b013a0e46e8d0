// inr_sense_place.h -- what the streaming kernels of inr_sense.hip and inr_sense_calib.hip share: the extents of a call,
// where pixel p of a plane lies under the shift, when two pixels move per access, and the launch size.
// Everything sits in an unnamed namespace: each translation unit gets its own copy, as when the text stood in
// inr_sense.hip itself.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace inr {

namespace {

constexpr int SN_THREADS = 64;
constexpr int SN_MAX_BLOCKS = 8192;  // 32 waves on each of 256 CUs

struct SenseDims {
  long long plane;   // H * W
  long long W;
  long long hh, hw;  // H / 2, W / 2
  long long H;
  int G, shift;
  float scale;
};

// where pixel p of a plane lies in x / gx
__device__ __forceinline__ long long sense_place(const SenseDims& d, long long p) {
  if (!d.shift) return p;
  long long y, x;
  if (d.plane <= 0xffffffffLL) {  // uniform: the 32-bit division is several times cheaper
    const unsigned pp = (unsigned)p, w = (unsigned)d.W;
    const unsigned yy = pp / w;
    y = yy, x = pp - yy * w;
  } else {
    y = p / d.W, x = p - y * d.W;
  }
  const long long ys = y >= d.hh ? y - d.hh : y - d.hh + d.H;
  const long long xs = x >= d.hw ? x - d.hw : x - d.hw + d.W;
  return ys * d.W + xs;
}

SenseDims sense_dims(int G, long long H, long long W, float scale, int shift) {
  SenseDims d;
  d.plane = H * W;
  d.W = W, d.H = H;
  d.hh = H / 2, d.hw = W / 2;
  d.G = G, d.shift = shift;
  d.scale = scale;
  return d;
}

bool sense_pairs(long long W, uintptr_t pointers) { return (pointers & 15u) == 0 && W % 2 == 0 && (W / 2) % 2 == 0; }

unsigned sense_blocks(long long units) {
  const long long b = (units + SN_THREADS - 1) / SN_THREADS;
  return (unsigned)(b < SN_MAX_BLOCKS ? b : SN_MAX_BLOCKS);
}

}  // namespace

}  // namespace inr
