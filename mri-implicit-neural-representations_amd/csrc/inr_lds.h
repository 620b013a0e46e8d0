// inr_lds.h -- where each piece of a kernel's dynamic LDS block lives: the one definition a kernel carves its
// `extern __shared__` block by and its launcher sizes the launch by.  One small struct per kernel family (inr_mlp_impl.h,
// inr_mlp_wide_impl.h, inr_mfn_impl.h / inr_mfn_wide_impl.h, inr_mlp_rs_impl.h, inr_siren_bf16_impl.h,
// inr_dw_gemm_bf16.hip), built from what the family knows (row blocks, waves or wave pairs, the encoder size); every piece
// has a named accessor that returns its offset from the block's start, bytes() is what the launch asks for.  The fp32
// kernels count in floats, the two bf16 kernels in bytes, as their code does.
//
// No HIP includes: tools/probes/lds_layout_check.cpp builds this with a host compiler and checks every instantiated shape
// for overlap, alignment and fit.
#pragma once
#include <cstddef>

#include "inr_hd.h"
#include "inr_w2.h"

// Row stride (floats) of a padded [feature][32 coordinates] LDS image.  36: 16-byte aligned rows (the dW A operand is then
// ONE ds_read_b128 per 4 k-steps, conflict-free because 36*i mod 64 walks all 16 four-bank slots); a translation unit whose
// images would not fit the CU that way defines 33 before its includes (inr_mfn_nb8.hip).
#ifndef INR_LDS_LD
#define INR_LDS_LD 36
#endif

namespace inr {

constexpr size_t LDS_BYTES_PER_CU = 160 * 1024;  // gfx950: what one workgroup may ask for (inr_launch.h refuses more)

// floats of the [E][3] encoder matrix, padded so that what follows it starts on 16 bytes
INR_HD constexpr int lds_enc_floats(int E) { return (3 * E + 3) & ~3; }
// floats of a [NB * 32 features][32 coordinates] image
INR_HD constexpr int lds_image_floats(int NB, int LD) { return NB * 32 * LD; }

// inr_mlp_kernel: one wave per 32 coordinates.  (floats)
//   [NW] images | encoder matrix (gauss input) | with ll: last-layer fragments | with dz: [NW] dZ_last images
// The block's first NW floats double as the waves' loss partials once the tiles are done.
struct MlpLds {
  int NB, NW, LD, EF;  // row blocks, waves, row stride, floats of the padded encoder matrix (0 without the fused encoder)

  INR_HD constexpr MlpLds(int nb, int nw, bool gauss, int E, int ld = INR_LDS_LD)
      : NB(nb), NW(nw), LD(ld), EF(gauss ? lds_enc_floats(E) : 0) {}

  INR_HD constexpr int image_floats() const { return lds_image_floats(NB, LD); }
  // MlpArgs::ll_lds: the last layer's fragments of output rows 0..3, [NB*4 groups][2 halves][4 rows] float4 + one of zeros
  INR_HD constexpr int last_frag_floats() const { return (NB * 4 * 8 + 1) * 4; }
  // MlpArgs::dz_lds: dZ_last [8][LD] of one wave
  INR_HD constexpr int dz_image_floats() const { return 8 * LD; }

  INR_HD constexpr int image(int w) const { return w * image_floats(); }
  INR_HD constexpr int enc() const { return NW * image_floats(); }
  INR_HD constexpr int last_frag() const { return enc() + EF; }
  INR_HD constexpr int dz_image(int w) const { return last_frag() + last_frag_floats() + w * dz_image_floats(); }

  // ll: with the fragments; dz: with the dZ_last images behind them (never without ll)
  INR_HD constexpr size_t bytes(bool ll, bool dz) const {
    return (size_t)(dz ? dz_image(NW) : (ll ? dz_image(0) : last_frag())) * sizeof(float);
  }
  // the options are taken where they fit; the launcher adds the network's own conditions (inr_mlp_impl.h, launch_mlp)
  INR_HD constexpr bool ll_fits() const { return bytes(true, false) <= LDS_BYTES_PER_CU; }
  INR_HD constexpr bool dz_fits() const { return bytes(true, true) <= LDS_BYTES_PER_CU; }
};

// inr_mlp_wide_kernel: a pair of waves per 32 coordinates, NG = 2 pairs.  (floats)
//   [NG] images | encoder matrix (gauss input) | eager: last-layer fragments | the pairs' exchange buffer [NG][4][32]
// eager: WIRE / WIRE2D, whose row owners form the activations once (WIDE_EAGER in inr_mlp_wide_impl.h)
struct MlpWideLds {
  static constexpr int NG = 2;
  int NB, LD, EF;
  bool eager;

  INR_HD constexpr MlpWideLds(int nb, bool gauss, int E, bool eager_, int ld = INR_LDS_LD)
      : NB(nb), LD(ld), EF(gauss ? lds_enc_floats(E) : 0), eager(eager_) {}

  INR_HD constexpr int image_floats() const { return lds_image_floats(NB, LD); }
  INR_HD constexpr int last_frag_floats() const { return NB * 4 * 8 * 4; }  // [NB*4 groups][2 halves][4 rows] float4
  INR_HD constexpr int pair_exchange_floats() const { return NG * 4 * 32; }

  INR_HD constexpr int image(int g) const { return g * image_floats(); }
  INR_HD constexpr int enc() const { return NG * image_floats(); }
  INR_HD constexpr int last_frag() const { return enc() + EF; }
  INR_HD constexpr int pair_exchange() const { return last_frag() + last_frag_floats(); }

  INR_HD constexpr size_t bytes() const {
    return (size_t)(eager ? pair_exchange() + pair_exchange_floats() : last_frag()) * sizeof(float);
  }
};

// inr_mfn_kernel (N = NW waves) and inr_mfn_wide_kernel (N = 2 wave pairs, NB = 16).  (floats)
//   [N] images | [N] head-gradient images [32][LD] | encoder matrix [E][3] (gauss input; nothing follows it: unpadded)
struct MfnLds {
  int NB, N, LD, EF;

  // (a kernel leaves gauss and E out: the encoder matrix is the last piece, only bytes() depends on it)
  INR_HD constexpr MfnLds(int nb, int n, bool gauss = false, int E = 0, int ld = INR_LDS_LD)
      : NB(nb), N(n), LD(ld), EF(gauss ? 3 * E : 0) {}

  INR_HD constexpr int image_floats() const { return lds_image_floats(NB, LD); }
  INR_HD constexpr int head_grad_floats() const { return lds_image_floats(1, LD); }

  INR_HD constexpr int image(int w) const { return w * image_floats(); }
  INR_HD constexpr int head_grad(int w) const { return N * image_floats() + w * head_grad_floats(); }
  INR_HD constexpr int enc() const { return head_grad(N); }

  INR_HD constexpr size_t bytes() const { return (size_t)(enc() + EF) * sizeof(float); }
};

// inr_mlp_rs_kernel: the row-split fused step.  (floats)
constexpr int RS_PITCH = 132;                  // floats per feature row of the LDS image: 16 jj x 8 c + 4
constexpr int RS_IMG_FLOATS = 256 * RS_PITCH;  // 135 168 B
constexpr int RS_MO_MAX = 4;                   // output rows the last layer computes at most: what a launch reserves

struct RsLds {
  int EF, MO;

  INR_HD constexpr explicit RsLds(int E, int mo = RS_MO_MAX) : EF(lds_enc_floats(E)), MO(mo) {}

  INR_HD constexpr int w_last_floats() const { return 4 * 256; }         // W_last [4][256], zero padded
  INR_HD constexpr int dz_last_floats() const { return 4 * 128; }        // dZ_last [4][128]
  INR_HD constexpr int red_floats() const { return 32; }                 // [32]: [8] sums of dZ_last | [4] loss partials
  INR_HD constexpr int part_floats() const { return 4 * MO * 128; }      // the waves' partial outputs [4][MO][128]

  INR_HD constexpr int image() const { return 0; }                       // [256][RS_PITCH]
  INR_HD constexpr int enc() const { return RS_IMG_FLOATS; }             // [E][3], padded
  INR_HD constexpr int w_last() const { return enc() + EF; }
  INR_HD constexpr int dz_last() const { return w_last() + w_last_floats(); }
  INR_HD constexpr int red() const { return dz_last() + dz_last_floats(); }
  INR_HD constexpr int part() const { return red() + red_floats(); }

  INR_HD constexpr size_t bytes() const { return (size_t)(part() + part_floats()) * sizeof(float); }
};

// inr_siren_bf16_kernel.  (BYTES)
//   ring of PN_SLOTS weight panels (filled by LDS-DMA) | bias table [D][256] | encoder matrix [E][4] | red [2][PN_WAVES]
constexpr int PN_SLOTS = 8;  // ring slots of W2_PANEL_BYTES
constexpr int PN_WAVES = 8;  // waves per workgroup; each moves 16 / 8 = 2 of a panel's 1 KB pieces

struct SirenBf16Lds {
  int D, E;  // Linear layers, encoder size

  INR_HD constexpr SirenBf16Lds(int d, int e) : D(d), E(e) {}

  INR_HD static constexpr int ring() { return 0; }
  INR_HD static constexpr int ring_end() { return PN_SLOTS * W2_PANEL_BYTES; }
  INR_HD constexpr int bias() const { return ring_end(); }                              // floats [D][256]
  INR_HD constexpr int enc() const { return bias() + D * 256 * (int)sizeof(float); }    // floats [E][4]: rows of 16 bytes
  INR_HD constexpr int red() const { return enc() + 4 * E * (int)sizeof(float); }       // floats [2][PN_WAVES]: loss
                                                                                        // partials, |dZ| maxima
  INR_HD constexpr size_t bytes() const { return (size_t)red() + 2 * PN_WAVES * sizeof(float); }
};

// dw_gemm_bf16_kernel.  (BYTES)
//   two stages of (A tile | B tile) in 2-byte elements | x of the stage's coordinates [2][GB_KS][3] | encoder matrix [E][3]
constexpr int GB_KS = 64;                // coordinates per stage
constexpr int GB_PITCH = 72;             // LDS row pitch in 2-byte elements: 64 coordinates + 16 bytes of padding
constexpr int GB_TILE = 256 * GB_PITCH;  // one operand tile (elements)
constexpr int GB_STAGE = 2 * GB_TILE;    // A tile + B tile

struct DwGemmBf16Lds {
  int E;

  INR_HD constexpr explicit DwGemmBf16Lds(int e) : E(e) {}

  INR_HD static constexpr int stage_bytes() { return GB_STAGE * 2; }
  INR_HD static constexpr int xs_bytes() { return 2 * GB_KS * 3 * (int)sizeof(float); }

  INR_HD static constexpr int stages() { return 0; }
  INR_HD static constexpr int xs() { return 2 * stage_bytes(); }
  INR_HD static constexpr int enc() { return xs() + xs_bytes(); }

  INR_HD constexpr size_t bytes() const { return (size_t)enc() + (size_t)3 * E * sizeof(float); }
};

}  // namespace inr
