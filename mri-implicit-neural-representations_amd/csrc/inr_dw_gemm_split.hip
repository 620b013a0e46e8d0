// inr_dw_gemm_split.hip -- the weight-gradient GEMM of inr_dw_gemm.hip (same arguments, items, chunks, slabs and stash
// layout; TL = 128, WB = 4 only) on the bf16 matrix pipe, with fp32 results.
//
// An fp32 number is exactly the sum of three bf16 numbers (24 significand bits = 8 + 8 + 8, same exponent range):
//   hi = x & 0xffff0000,  r = x - hi (exact),  mid = r & 0xffff0000,  lo = r - mid (exact, <= 8 significant bits),
// and a bf16 x bf16 product is exact in fp32.  With a = a1 + a2 + a3 and b = b1 + b2 + b3 the six products
//   a1 b1,  a1 b2,  a2 b1,  a2 b2,  a1 b3,  a3 b1
// leave out terms <= 2^-24 |a b| -- one fp32 rounding.  a1 b1 is summed in one fp32 accumulator set and the five
// corrections in a second one; the two are added once in front of the slab store, so that the corrections are not
// rounded against the large running sum at every MFMA.  Six v_mfma_f32_32x32x16_bf16 (32 cycles each for K = 16) replace
// eight v_mfma_f32_32x32x2_f32 (64 cycles each): 0.375 of the matrix-pipe time.
//
// Workgroup = a 128 x 256 block of one item's dW over one chunk of tiles, four waves 2 x 2, each 64 x 128 = 2 x 4 MFMA
// blocks x two accumulator sets = 256 registers.  (Plans with 256 x 256 tiles, WBM = 0: two such workgroups per tile.)
// A stage = 32 coordinates of 384 operand rows.  LDS image of a stage: row pitch 208 bytes = three planes (hi, mid, lo) of
// 32 bf16 + 16 bytes of padding: 13 sixteen-byte slots, odd, so the ds_read_b128 fragments of 16 consecutive rows fall
// into 16 distinct slots of the 256-byte bank row.  Two stage buffers: 2 x 79 872 bytes.
//
// The stage loop is one software-pipelined basic block of twelve slots of 8 MFMAs (one product of one K = 16 group).
// Slot h also splits the h-th of the thread's twelve 16-byte operand pieces of the NEXT stage into the other LDS buffer
// (22 vector instructions, three ds_write_b64) and then fetches the same piece of the stage after that into the freed
// registers: every global load has a whole stage to arrive, with one register set.  Fragments are single-buffered: the
// order  a2b2, a1b2, a1b3, a1b1, a2b1, a3b1  frees a plane at least one slot (256 matrix-pipe cycles) before the next
// K = 16 group's product needs it, and the last product of a stage is multiplied after the barrier, under the first
// fragment reads of the next stage.  db: fp32 sums of the unsplit dZ, taken where the pieces are split.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "inr_dw_gemm.h"
#include "inr_dw_place.h"
#include "inr_stamp_rt.h"
#include "inr_launch.h"

namespace inr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int SP_TL = 128;                     // coordinates per stash slot
constexpr int SP_KS = SP_TL / 32;              // stages per slot
constexpr int SP_GROWS = 128, SP_HROWS = 256;  // rows of the dZ tile and of the h tile
constexpr int SP_NF = (SP_GROWS + SP_HROWS) / 32;  // 16-byte pieces per thread and stage
constexpr int SP_PLANE = 64;                   // bytes of one bf16 plane of a row (32 coordinates)
constexpr int SP_PITCH = 3 * SP_PLANE + 16;    // bytes per LDS row
constexpr int SP_STAGE = (SP_GROWS + SP_HROWS) * SP_PITCH;

// the schedule of one slot: each of the 8 MFMAs is followed by its share of the slot's other instructions
template <int NREAD, int LEAD = 0, int M = 0>
__device__ __forceinline__ void sp_sched() {
  if constexpr (M == 0 && LEAD > 0) __builtin_amdgcn_sched_group_barrier(0x100, LEAD, 0);  // reads the next slot waits for
  if constexpr (M < 8) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (M < NREAD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // a fragment read
    __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);                           // split arithmetic
    if constexpr (M >= 5) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);     // a plane of the split piece
    if constexpr (M == 7) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);     // the piece's next fetch
    sp_sched<NREAD, LEAD, M + 1>();
  }
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t sp_rsrc(const float* p) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0, 0x7ffffff0, 0x00020000);
}

// four consecutive coordinates of one row -> their hi / mid / lo bf16 planes at dst; SUM: flag * (their sum) joins bs
template <bool SUM>
__device__ __forceinline__ void sp_split_store(char* dst, const f32x4& x, float& bs, float flag) {
  unsigned xb[4], rb[4], lb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float xe = x[e];  // (a scalar copy: __builtin_bit_cast of the vector element itself reads element 0)
    xb[e] = __builtin_bit_cast(unsigned, xe);
    const float r = xe - __builtin_bit_cast(float, xb[e] & 0xffff0000u);
    rb[e] = __builtin_bit_cast(unsigned, r);
    lb[e] = __builtin_bit_cast(unsigned, r - __builtin_bit_cast(float, rb[e] & 0xffff0000u));
    if (SUM) bs = fmaf(xe, flag, bs);
  }
  // the upper halves of two dwords, side by side
  const u32x2 h = {__builtin_amdgcn_perm(xb[1], xb[0], 0x07060302u), __builtin_amdgcn_perm(xb[3], xb[2], 0x07060302u)};
  const u32x2 m = {__builtin_amdgcn_perm(rb[1], rb[0], 0x07060302u), __builtin_amdgcn_perm(rb[3], rb[2], 0x07060302u)};
  const u32x2 l = {__builtin_amdgcn_perm(lb[1], lb[0], 0x07060302u), __builtin_amdgcn_perm(lb[3], lb[2], 0x07060302u)};
  *reinterpret_cast<u32x2*>(dst) = h;
  *reinterpret_cast<u32x2*>(dst + SP_PLANE) = m;
  *reinterpret_cast<u32x2*>(dst + 2 * SP_PLANE) = l;
}

// mb0 / nb0: first 32-row block of dZ / of h of this workgroup's 128 x 256 block
template <bool BIAS>
__device__ __forceinline__ void sp_body(const DwGemmArgs& a, const DwGemmItem& it, int kc, int mb0, int nb0, char* lds) {
  constexpr int NF = SP_NF;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int half = lane >> 5, li = lane & 31;
  const int wm = w >> 1, wn = w & 1;
  f32x16 acc0[2][4], acc1[2][4];  // a1 b1; the five corrections
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[i][j][r] = 0.f, acc1[i][j][r] = 0.f;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  // loader: piece k of thread t = coordinates 4 seg .. + 3 of row prow + 32 k ([0, 128): dZ, [128, 384): h).  The four
  // 8-lane groups of a 32-lane write go to rows 4 apart: 4 x 208 bytes = 64 mod 256, four disjoint 64-byte windows.
  const int seg = t & 7, q = t >> 3;
  const int prow = ((q & 3) << 2) | ((q >> 2) & 3) | (q & 16);
  int roff[NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const bool isg = k < SP_GROWS / 32;
    const int blk = isg ? mb0 + k : nb0 + (k - SP_GROWS / 32);
    const int row = (blk < (isg ? it.Mblk : it.Kblk)) ? blk * 32 + prow : 0;  // rows past a tensor's extent: row 0, never stored
    roff[k] = ((isg ? it.g_off : it.h_off) + row * SP_TL + seg * 4) * 4;      // bytes
  }
  char* wr = lds + prow * SP_PITCH + seg * 8;
  const int t0 = a.tile0 + kc * a.tiles_per_chunk;
  int n_mine = a.n_tiles - t0;
  if (n_mine > a.tiles_per_chunk) n_mine = a.tiles_per_chunk;
  const int n_steps = (n_mine > 0 ? n_mine : 0) * SP_KS;
  auto stage_ptr = [&](int s) -> const float* {  // operands of stage s (past the end: the last stage again, never multiplied)
    const int sf = s < n_steps ? s : n_steps - 1;
    return a.save + (size_t)(t0 + sf / SP_KS) * a.save_floats_per_tile + 32 * (sf % SP_KS);
  };
  const char* As = lds + (wm * 64 + li) * SP_PITCH + 16 * half;
  const char* Bs = lds + (SP_GROWS + wn * 128 + li) * SP_PITCH + 16 * half;
  // fragments: plane p (0: hi, 1: mid, 2: lo)
  u32x4 A[3][2], B[3][4];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
#pragma unroll
    for (int i = 0; i < 2; ++i) A[p][i] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) B[p][j] = u32x4{0u, 0u, 0u, 0u};
  }
  auto rdA = [&](int p, int g, const char* Ab) {
#pragma unroll
    for (int i = 0; i < 2; ++i) A[p][i] = *reinterpret_cast<const u32x4*>(Ab + i * 32 * SP_PITCH + p * SP_PLANE + 32 * g);
  };
  auto rdB = [&](int p, int g, const char* Bb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) B[p][j] = *reinterpret_cast<const u32x4*>(Bb + j * 32 * SP_PITCH + p * SP_PLANE + 32 * g);
  };
  auto prod = [&](int pa, int pb, f32x16 (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A[pa][i]),
                                                            __builtin_bit_cast(bf16x8, B[pb][j]), acc[i][j], 0, 0, 0);
  };
  f32x4 v[NF];
  if (n_steps > 0) {  // (an empty chunk still writes its zeros)
    const __amdgpu_buffer_rsrc_t r0 = sp_rsrc(stage_ptr(0)), r1 = sp_rsrc(stage_ptr(1));
#pragma unroll
    for (int k = 0; k < NF; ++k) v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r0, roff[k], 0, 0));
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      if (BIAS && k < 4)
        sp_split_store<true>(wr + k * 32 * SP_PITCH, v[k], bsum[k], 1.f);
      else
        sp_split_store<false>(wr + k * 32 * SP_PITCH, v[k], bsum[0], 0.f);
      v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r1, roff[k], 0, 0));
    }
  }
  // descriptor of the stage the loop fetches (s + 2): formed at the END of the stage before, in front of the barrier's own
  // wait -- at the top of a stage its scalar arithmetic drew a wait for every LDS read in flight
  __amdgpu_buffer_rsrc_t rs = sp_rsrc(stage_ptr(2));
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < n_steps; ++s) {
    const char* Ab = As + (s & 1) * SP_STAGE;
    const char* Bb = Bs + (s & 1) * SP_STAGE;
    char* wb = wr + ((s + 1) & 1) * SP_STAGE;
    const float flag = s + 1 < n_steps ? 1.f : 0.f;
    // piece h of stage s + 1 into LDS, then piece h of stage s + 2 into its registers
    auto piece = [&](auto H) {
      constexpr int h = decltype(H)::value;
      if constexpr (BIAS && h < 4)
        sp_split_store<true>(wb + h * 32 * SP_PITCH, v[h], bsum[h], flag);
      else
        sp_split_store<false>(wb + h * 32 * SP_PITCH, v[h], bsum[0], 0.f);
      v[h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, roff[h], 0, 0));
    };
#define SP_SLOT(H, NREAD, LEAD, ...)                       \
  do {                                                 \
    __VA_ARGS__;                                       \
    piece(std::integral_constant<int, H>{});           \
    sp_sched<NREAD, LEAD>();                           \
    __builtin_amdgcn_sched_barrier(0);                 \
  } while (0)
    // the previous stage's last product (zeros in front of stage 0) under the first reads of this stage
    rdA(1, 0, Ab), rdB(1, 0, Bb), rdA(0, 0, Ab);
    SP_SLOT(0, 0, 12, rdB(2, 0, Bb); prod(2, 0, acc1));
    // K = 16 group 0; behind a product: the planes it was the last to use, from group 1
    SP_SLOT(1, 6, 0, rdA(2, 0, Ab); rdB(0, 0, Bb); prod(1, 1, acc1));
    SP_SLOT(2, 0, 0, prod(0, 1, acc1));
    SP_SLOT(3, 4, 0, rdB(1, 1, Bb); prod(0, 2, acc1));
    SP_SLOT(4, 4, 0, rdB(2, 1, Bb); prod(0, 0, acc0));
    SP_SLOT(5, 2, 0, rdA(0, 1, Ab); prod(1, 0, acc1));
    SP_SLOT(6, 2, 0, rdA(1, 1, Ab); prod(2, 0, acc1));
    // K = 16 group 1 (its a3 b1 waits for the barrier)
    SP_SLOT(7, 6, 0, rdA(2, 1, Ab); rdB(0, 1, Bb); prod(1, 1, acc1));
    SP_SLOT(8, 0, 0, prod(0, 1, acc1));
    SP_SLOT(9, 0, 0, prod(0, 2, acc1));
    SP_SLOT(10, 0, 0, prod(0, 0, acc0));
    SP_SLOT(11, 0, 0, prod(1, 0, acc1));
#undef SP_SLOT
    rs = sp_rsrc(stage_ptr(s + 3));
    __syncthreads();
  }
  prod(2, 0, acc1);  // the last stage's a3 b1
  float* slab = a.slabs + (size_t)kc * a.slab_floats;
  const int mb = mb0 + 2 * wm, nb = nb0 + 4 * wn;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (mb + i >= it.Mblk) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int colj = 32 * (nb + j) + li;
      if (colj < it.K) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * (mb + i) + (r & 3) + 8 * (r >> 2) + 4 * half;
          slab[it.gw_off + (size_t)row * it.K + colj] = acc0[i][j][r] + acc1[i][j][r];
        }
      }
    }
  }
  if (BIAS) {  // the 8 threads of a row (consecutive lanes) hold the sums of their 4-coordinate segments
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float tot = bsum[k];
      tot += __shfl_xor(tot, 1);
      tot += __shfl_xor(tot, 2);
      tot += __shfl_xor(tot, 4);
      if (seg == 0 && mb0 + k < it.Mblk) slab[it.gb_off + 32 * (mb0 + k) + prow] = tot;
    }
  }
}

// SPLITM: workgroups per workgroup tile of the plan (1: 128 x 256 tiles, WBM = 2; 2: 256 x 256 tiles)
template <int SPLITM>
__global__ __launch_bounds__(256) void dw_gemm_split_kernel(const DwGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds_split[];
  INR_RT_STAMP(a.dbg, a.dbg_cap, 4, threadIdx.x >> 6, threadIdx.x & 63, 44);
  const int bpc = a.blocks_per_chunk * SPLITM;
  // a chunk's workgroups read the same stash rows: place them under one L2 (inr_dw_place.h); a.place == 0: in id order
  const int b = a.place ? dw_place((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int kc = b / bpc;
  const int rem = b - kc * bpc;
  const int unit = rem / SPLITM, hh = rem - unit * SPLITM;
  int k = 0;
  while (k + 1 < a.n_items && unit >= a.it[k + 1].unit0) ++k;
  const DwGemmItem& it = a.it[k];
  const int u = unit - it.unit0;
  const int mi = u / it.nt, ni = u % it.nt;
  const int mb0 = 4 * (SPLITM * mi + hh);
  if (mb0 < it.Mblk) {  // (the lower half of a 256-row tile over a tensor of 128 rows has nothing to store)
    if (ni == 0)
      sp_body<true>(a, it, kc, mb0, 0, lds_split);
    else
      sp_body<false>(a, it, kc, mb0, 8 * ni, lds_split);
  }
  INR_RT_STAMP(a.dbg, a.dbg_cap, 4, threadIdx.x >> 6, threadIdx.x & 63, 45);
}

template <int SPLITM>
static hipError_t launch_split(const DwGemmArgs& a, hipStream_t st) {
  constexpr size_t lds_bytes = (size_t)2 * SP_STAGE;
  static_assert(lds_bytes <= LDS_BYTES_PER_CU, "two stage buffers must fit the CU's LDS");
  const dim3 grid((unsigned)(a.n_chunks * a.blocks_per_chunk * SPLITM));
  return launch_lds<dw_gemm_split_kernel<SPLITM>>(grid, dim3(256), lds_bytes, st, a);
}

// called by launch_dw_gemm with units / blocks_per_chunk / stamps filled in
hipError_t launch_dw_gemm_split(const DwGemmArgs& a, hipStream_t st) {
  if (a.TL != SP_TL || a.WB != 4) return hipErrorInvalidValue;
  const int wbm = a.WBM > 0 ? a.WBM : a.WB;
  if (wbm == 2) return launch_split<1>(a, st);
  if (wbm == 4) return launch_split<2>(a, st);
  return hipErrorInvalidValue;
}

}  // namespace inr
