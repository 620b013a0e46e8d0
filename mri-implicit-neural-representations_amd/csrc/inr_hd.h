// inr_hd.h -- INR_HD: marks the layout functions that kernels and the host share (inr_w2.h, inr_stash.h).  Empty under a
// plain C++ compiler, so those headers also build into host-only probes.
#pragma once

#if defined(__HIPCC__)
#define INR_HD __host__ __device__
#else
#define INR_HD
#endif
