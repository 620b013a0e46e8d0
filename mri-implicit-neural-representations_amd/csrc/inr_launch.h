// inr_launch.h -- host-side launch helpers shared by every kernel translation unit: the one place a kernel with dynamic
// LDS is launched from (how many bytes, and where each piece lives inside them: inr_lds.h)
#pragma once
#include <hip/hip_runtime.h>

#include "inr_lds.h"

// Kernels with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised once per
// (kernel, DEVICE): a process may drive plans on several GPUs from one thread, so the "already done" bit is kept
// per device ordinal (one static word per kernel instantiation; bit d = device d).
#include <atomic>
namespace inr {
template <auto Kernel>
inline hipError_t allow_full_lds() {
  static std::atomic<unsigned long long> done{0ull};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_relaxed) >> dev) & 1ull)) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)LDS_BYTES_PER_CU);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_relaxed);
  return hipSuccess;
}

// How every kernel with dynamic LDS starts: a block larger than the CU's LDS is refused here, on the host, before
// anything reaches the device.
template <auto Kernel, class... Args>
inline hipError_t launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args&... args) {
  if (lds_bytes > LDS_BYTES_PER_CU) return hipErrorInvalidValue;
  hipError_t e = allow_full_lds<Kernel>();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
  return hipGetLastError();
}
}  // namespace inr
