// inr_stash.h -- where each tensor of the fp32 activation stash (the `save` workspace) lives inside one tile's slot.
// The one definition the fused kernels (inr_mlp_impl.h, inr_mlp_wide_impl.h, inr_mlp_rs_impl.h, inr_mfn_impl.h,
// inr_mfn_wide_impl.h), the weight-gradient GEMM's items and the plan's stash size (inr_plan.hip) share.  The bf16 path's
// 8-bit stash is inr_w2.h's.
//
// A tile's slot is a sequence of TENSORS of [NB * 32 feature rows][TL coordinates] floats, a few per hidden layer
// (MlpStash) or per stage (MfnStash), then the smaller pieces.  All offsets are in floats from the slot's start; every
// piece starts at a multiple of TL floats, so a row of any tensor may be read 16 bytes at a time.
//
// No HIP includes: tools/probes/stash_layout_check.cpp builds this with a host compiler.
#pragma once
#include <cstddef>

#include "inr_hd.h"

namespace inr {

// floats of one stashed tensor
INR_HD constexpr int stash_tensor_floats(int NB, int TL) { return NB * 32 * TL; }

// Activation family of a plain MLP; the value is the number of tensors it stashes per hidden layer.
enum StashFamily {
  STASH_REAL = 2,     // SIREN / FFN: h, act'
  STASH_GABOR = 3,    // WIRE: h, dA, dB
  STASH_GABOR2D = 7,  // WIRE2D: h, dA, dB, dA2, dB2, orth, u^2+v^2
};

// SIREN / FFN / WIRE / WIRE2D; the one-wave-per-group, two-waves-per-group and row-split kernels.
//   [hidden layer 0 .. D-2][slot] tensors | act'(z_last) [4][TL] | encoder features [enc_rows][TL] (gauss input)
//                                                                | copy of a layer's output gradient, one tensor (WIRE2D)
struct MlpStash {
  int NB, TL, NS, T;  // row blocks, coordinates per tile, tensors per hidden layer, floats per tensor

  // slots of a hidden layer (rows of complex layers are interleaved (Re, Im) pairs)
  enum Slot {
    H = 0,     // the layer's output h_l (the activation y_l)
    DACT = 1,  // real activations: act'(z_l).  Backward overwrites it IN PLACE with dZ_l = dH_l * act'(z_l): from then on
               // the slot is the A operand of the batch weight-gradient GEMM (the same holds for DA)
    DA = 1,    // complex activations: the Jacobian's factors of the (Re, Im) parts of dH_l; where the wavelet is formed
    DB = 2,    // eagerly by the row owners (two waves per group) DA holds the pre-activation z_l = a + j b instead, from
               // which (with y_l in H) the Jacobian is formed again in backward, and DB stays unwritten
    DA2 = 3,   // WIRE2D: the same factors for the layer's second Linear; DA2 becomes dZ_orth,l in place
    DB2 = 4,
    ORTH = 5,  // WIRE2D: the second Linear's output (u, v)
    Q = 6,     // WIRE2D: u^2 + v^2
  };

  INR_HD constexpr MlpStash(int nb, int tl, StashFamily family)
      : NB(nb), TL(tl), NS(family), T(stash_tensor_floats(nb, tl)) {}

  // D: the network's Linear layers (hidden layers 0 .. D-2)
  INR_HD constexpr int tensor_floats() const { return T; }
  INR_HD constexpr size_t slot(int l, int s) const { return (size_t)(NS * l + s) * T; }
  // [4][TL]: act'(z_last) of output rows 0..3, kept by a forward call for its backward call
  INR_HD constexpr size_t last_dact(int D) const { return (size_t)NS * (D - 1) * T; }
  // encoder features [enc_rows][TL] of the fused gauss encoder, and WIRE2D's copy of dH_l [NB*32][TL], start at the SAME
  // offset: no plan has both (inr_plan_create refuses WIRE / WIRE2D behind the gauss encoder)
  INR_HD constexpr size_t enc(int D) const { return last_dact(D) + 4 * TL; }
  INR_HD constexpr size_t grad_copy(int D) const { return enc(D); }
  // enc_rows: rows of the encoder-feature image (32 per k-block of layer 0), 0 without the fused encoder
  INR_HD constexpr size_t floats_per_tile(int D, int enc_rows) const {
    return enc(D) + (size_t)enc_rows * TL + (NS == STASH_GABOR2D ? T : 0);
  }
};

// Multiplicative filter networks, both kernels.
//   [stage 0 .. S-1][slot] tensors | input features [enc_rows][TL] | |x|^2 [TL] (read by the Gabor filters)
struct MfnStash {
  int NB, TL, T;  // row blocks, coordinates per tile, floats per tensor

  enum Slot {
    F = 0,     // f_i = sin(u_i) (times the Gabor envelope).  The 512-wide kernel's backward overwrites it in place with
               // g_l = g_h * f, the A operand of dL_{i-1}
    LCOS = 1,  // l_i cos u_i; becomes g_u = g_h * l cos u in place, the A operand of dF_i
    HH = 2,    // the stage's output h_i
  };

  INR_HD constexpr MfnStash(int nb, int tl) : NB(nb), TL(tl), T(stash_tensor_floats(nb, tl)) {}

  // S: live stages; enc_rows: rows of the input-feature image (32 per k-block of a filter)
  INR_HD constexpr int tensor_floats() const { return T; }
  INR_HD constexpr size_t slot(int stage, int s) const { return ((size_t)3 * stage + s) * T; }
  INR_HD constexpr size_t enc(int S) const { return (size_t)3 * S * T; }
  INR_HD constexpr size_t x2(int S, size_t enc_rows) const { return enc(S) + enc_rows * TL; }
  INR_HD constexpr size_t floats_per_tile(int S, size_t enc_rows) const { return x2(S, enc_rows) + TL; }
};

}  // namespace inr
