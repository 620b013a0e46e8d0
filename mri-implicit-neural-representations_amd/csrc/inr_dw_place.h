// inr_dw_place.h -- which piece of the weight-gradient GEMM's work a block id takes (inr_dw_gemm_split.hip).
//
// Block ids are dealt round-robin to the 8 XCDs, each with an L2 of its own: ids b and b + 8 share an L2, b and b + 1
// do not.  The workgroups of one chunk read the same stash rows (the two M-halves of a layer all of h, the n-tiles of
// layer 0 the same dZ), so the ids of one residue class mod 8 get a CONTIGUOUS range of logical ids: whole chunks,
// apart from the at most 7 chunks that straddle the boundary between two classes.  The map is a bijection of [0, G)
// for every G (classes below G % 8 hold one id more); b % 8 only labels "shares an L2" -- the result does not depend
// on it, every logical id computes and stores what it always did.
//
// No HIP includes: tools/probes/dw_place_check.cpp builds this with a host compiler.
#pragma once

#ifdef __HIPCC__
#define INR_DW_PLACE_FN __host__ __device__ inline
#else
#define INR_DW_PLACE_FN inline
#endif

namespace inr {

constexpr int DW_PLACE_XCDS = 8;

// logical id of block b of a grid of G blocks
INR_DW_PLACE_FN int dw_place(int b, int G) {
  const int x = b % DW_PLACE_XCDS, j = b / DW_PLACE_XCDS;
  const int q = G / DW_PLACE_XCDS, r = G % DW_PLACE_XCDS;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

}  // namespace inr

#undef INR_DW_PLACE_FN
