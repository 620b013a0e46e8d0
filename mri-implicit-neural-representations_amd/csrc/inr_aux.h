// inr_aux.h -- host-side launchers shared between the translation units of libinr_mi355x.so
#pragma once
#include "inr_device.h"
#include "inr_mlp_args.h"

namespace inr {

// ---- the tail of a training step (inr_params.hip): slab reduction, Adam + re-pack, penalty gradients ----
// The weight images of `packed` as three sets (bits): inr_mlp_kernel's forward and transposed images, and the row-split
// kernel's fragment images.  Bias tables and the bf16 panel stream belong to no set: every update writes them.
enum { IMG_FWD = 1, IMG_TR = 2, IMG_RS = 4, IMG_ALL = 7 };

struct AdamArgs {
  int do_update;      // 0: pack only
  int skip_sets;      // IMG_* sets of a row-split plan's images this launch leaves alone (0: every image is written)
  int all_real;       // set by the launcher: every layer is LT_REAL or LT_GABOR_MU (fast scatter path)
  int flat_order;     // set by the launcher: ... and the layers lie in the flat vector in L[] order (layer_walk, inr_params.hip)
  int has_dead;       // set by the launcher (adam_dead_ranges): some layer has live == 0 ...
  int n_dead;         // ... and its flat entries are these merged ranges [dead_lo, dead_hi); -1: more than fit, walk the layers
  int dead_lo[8], dead_hi[8];
  float step_size;    // lr / (1 - beta1^t), computed in double on the host like torch does
  float bc2_sqrt;     // sqrt(1 - beta2^t)
  float omb1;         // float(1 - beta1): the lerp weight torch passes to exp_avg.lerp_
  float beta2, omb2;  // float(beta2), float(1 - beta2)
  float eps, weight_decay, l1, l2;
  // graph-replayable form (inr_adam_step_dev): the step is read from device memory and indexes a table of
  // (step_size, bc2_sqrt) pairs, so that no kernel argument changes from one step to the next
  const float* sched;   // nullptr: use step_size / bc2_sqrt above
  const int* step_dev;  // steps taken so far
  int n_sched;
};

// entries of the layers in `mask` (bit l = L[l]) and the flat gradient entries [lo, hi) are summed over the n2 slabs
// that FOLLOW the n_blocks slabs of the fused kernel (partial sums of the batch-level weight-gradient GEMM);
// n2 == 0: one slab set
// ... and, of those, the flat entries [lo3, hi3) over n3 slabs of the same set instead of n2 (the bf16 GEMM gives its
// first-layer units, whose operand is arithmetic rather than a load, shorter chunks -- more of them; n3 == 0: none)
struct SlabSplit {
  int lo, hi, n2;
  unsigned mask;
  int lo3 = 0, hi3 = 0, n3 = 0;
};
hipError_t launch_reduce_slabs(const NetDesc& nd, const float* slabs, int n_blocks, float* grads, float* loss_out,
                               const float* params, const float* packed, hipStream_t st,
                               SlabSplit split = SlabSplit{0, 0, 0, 0});
hipError_t launch_step_advance(int* step_dev, hipStream_t st);
hipError_t launch_reduce_slabs_adam(const NetDesc& nd, const float* slabs, int n_blocks, float* grads, float* loss_out,
                                    float* params, float* m1, float* m2, float* packed, const AdamArgs& aa,
                                    hipStream_t st, SlabSplit split);
hipError_t launch_reg_grad(const NetDesc& nd, const float* params, float* grads, int lo, int hi, float l1, float l2,
                           const float* l2_dir, hipStream_t st);
hipError_t launch_adam_shard(const NetDesc& nd, float* params, const float* grads_shard, float* m1, float* m2, int lo,
                             int hi, const AdamArgs& aa, hipStream_t st);
hipError_t launch_adam_pack(const NetDesc& nd, float* params, const float* grads, float* m1, float* m2,
                            float* packed, const AdamArgs& aa, hipStream_t st);
// ---- the stand-alone positional encoders (inr_encode.hip) ----
hipError_t launch_encode_logf(const float* coords, const float* bands, long long B, int nb, float* out,
                              hipStream_t st);
hipError_t launch_encode_gauss(const float* coords, const float* encB, long long B, int E, float* out,
                               hipStream_t st);
// ---- losses on the network output and their gradients (inr_loss.hip) ----
hipError_t launch_loss_grad(const LossDesc& ld, const float* out, const float* gt, const uint8_t* mask, long long B,
                            float* loss_out, float* dout, hipStream_t st);
hipError_t launch_loss_grad_multi(const LossDesc& ld, const float* outs, const float* gt, const float* dist,
                                  const uint8_t* mask, int NH, long long B, float* loss_out, float* douts,
                                  hipStream_t st);
// CenterLoss random-pair term (losses.py:175-199): adds w * sum_p r_p^2 to loss_out[0] and its gradient to dout
hipError_t launch_center_pairs(const float* out, const float* gt, const long long* ia, const long long* ib, long long n,
                               long long B, float w, float* loss_out, float* dout, hipStream_t st);
hipError_t launch_loss_tv_grad(const LossDesc& ld, const float* out, const float* gt, const uint8_t* mask, long long R,
                               long long R_own, long long W, float cw, float ch, float* loss_out, float* dout,
                               hipStream_t st);
hipError_t launch_tv_grad(const float* out, long long R, long long R_own, long long W, float cw, float ch,
                          float* loss_out, float* dout, hipStream_t st);

// ---- the fused network kernels: one translation unit per (family, hidden block count NB) / per row-split width ----
// mode 0 fwd, 1 bwd, 2 fused
using NetLaunch = hipError_t(const NetDesc& nd, const LossDesc& ld, const MlpArgs& a, int mode, int grid, hipStream_t st);
using StepLaunch = hipError_t(const NetDesc& nd, const LossDesc& ld, const MlpArgs& a, int grid, hipStream_t st);
NetLaunch launch_mlp_nb1, launch_mlp_nb2, launch_mlp_nb4, launch_mlp_nb8, launch_mlp_nb16, launch_siren_bf16;
NetLaunch launch_wire_nb2, launch_wire_nb4, launch_wire_nb8, launch_wire_nb12;
NetLaunch launch_wire2d_nb2, launch_wire2d_nb4, launch_wire2d_nb8, launch_wire2d_nb16;
NetLaunch launch_mfn_nb1, launch_mfn_nb4, launch_mfn_nb8, launch_mfn_nb16;
StepLaunch launch_siren_bf16_fwd, launch_siren_bf16_bwd, launch_siren_bf16_fused;
// row-split fused step, tiles of N column blocks of 16 coordinates (inr_mlp_rs_n*.hip)
StepLaunch launch_mlp_rs_n1, launch_mlp_rs_n2, launch_mlp_rs_n3, launch_mlp_rs_n4, launch_mlp_rs_n5, launch_mlp_rs_n6,
    launch_mlp_rs_n7;

// The kernel of a plan: its family's build for nd.NB -- the family's LAST row (its largest build) for any other NB.
// bf16 plans: weight panels in LDS, dW by inr_dw_gemm_bf16.hip.
enum NetFamily { FAM_MFN, FAM_WIRE2D, FAM_WIRE, FAM_BF16, FAM_MLP };
inline NetLaunch* net_kernel(const NetDesc& nd) {
  static constexpr struct {
    NetFamily fam;
    int NB;
    NetLaunch* fn;
  } built[] = {
      {FAM_MFN, 1, launch_mfn_nb1}, {FAM_MFN, 4, launch_mfn_nb4}, {FAM_MFN, 8, launch_mfn_nb8}, {FAM_MFN, 16, launch_mfn_nb16},
      {FAM_WIRE2D, 2, launch_wire2d_nb2}, {FAM_WIRE2D, 4, launch_wire2d_nb4}, {FAM_WIRE2D, 8, launch_wire2d_nb8},
      {FAM_WIRE2D, 16, launch_wire2d_nb16},
      {FAM_WIRE, 2, launch_wire_nb2}, {FAM_WIRE, 4, launch_wire_nb4}, {FAM_WIRE, 8, launch_wire_nb8}, {FAM_WIRE, 12, launch_wire_nb12},
      {FAM_BF16, 8, launch_siren_bf16},
      {FAM_MLP, 1, launch_mlp_nb1}, {FAM_MLP, 2, launch_mlp_nb2}, {FAM_MLP, 4, launch_mlp_nb4}, {FAM_MLP, 8, launch_mlp_nb8},
      {FAM_MLP, 16, launch_mlp_nb16},
  };
  const NetFamily fam = nd.mfn_n > 0 ? FAM_MFN
                        : nd.hact == ACT_GABOR2D ? FAM_WIRE2D
                        : nd.hact == ACT_GABOR ? FAM_WIRE
                        : nd.bf16 ? FAM_BF16 : FAM_MLP;
  NetLaunch* fn = nullptr;
  for (const auto& k : built)
    if (k.fam == fam) {
      fn = k.fn;
      if (k.NB == nd.NB) break;
    }
  return fn;
}
// ... and the row-split kernel for tiles of `ncb` column blocks (anything outside 1..6: the widest build)
inline StepLaunch* rs_kernel(int ncb) {
  static constexpr StepLaunch* built[] = {launch_mlp_rs_n1, launch_mlp_rs_n2, launch_mlp_rs_n3, launch_mlp_rs_n4,
                                          launch_mlp_rs_n5, launch_mlp_rs_n6, launch_mlp_rs_n7};
  return built[ncb >= 1 && ncb <= 6 ? ncb - 1 : 6];
}

// image metrics of the validation epoch (inr_eval.hip): RSS over coils, then PSNR / SSIM against `ref` when it is given
long long image_metrics_scratch_doubles(long long H, long long W);
hipError_t launch_image_metrics(const float* coils, int C, int H, int W, const float* ref, float* rss_out,
                                double* metrics_out, double* scratch, hipStream_t st);

// pictures and per-coil table of the validation epoch (inr_display.hip)
long long kspace_display_scratch_floats(long long H, long long W);
hipError_t launch_kspace_display(const float* coils, const float* minus, int C, int H, int W, float expm1_sf, float* out,
                                 float* scratch, hipStream_t st);
long long gray8_scratch_floats(long long H, long long W);
hipError_t launch_gray8(const float* img, int H, int W, int take_abs, int has_range, float vmin, float vmax,
                        const unsigned char* lut, unsigned char* out, float* norm_out, float* scratch, hipStream_t st);
long long coil_stats_scratch_doubles(long long C, long long H, long long W);
hipError_t launch_coil_stats(const float* coils, int C, int H, int W, double* stats, double* scratch, hipStream_t st);

// shuffled epochs (inr_shuffle.hip): round keys of (seed, epoch) and the half width of the Feistel
// domain, both made on the host (inr_api_aux.hip shuffle_keys)
#define SHUFFLE_ROUNDS 6
struct ShuffleKeys {
  unsigned k[SHUFFLE_ROUNDS];
  int h;
};
// the mixer of the key schedule (host) and of the round function (device): inr_mi355x/shuffle.py::_mix
__host__ __device__ inline unsigned shuffle_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
hipError_t launch_shuffle_epoch(const ShuffleKeys& sk, long long n, long long bs, const float* coords, const float* gt,
                                const float* dist, const uint8_t* mask, float* coords_out, float* gt_out, float* dist_out,
                                uint8_t* mask_out, int* batch_counts, long long* order_out, hipStream_t st);

// weighted epochs (inr_sample.hip): the integer CDF of per-row ticks and the stratified draw from it.
// sk permutes the m strata ([0, m), not [0, n)); dk are the two keys of a stratum's offset (inr_api_aux.hip draw_keys)
struct DrawKeys {
  unsigned k[2];
};
long long row_cdf_scratch_words(long long n);
hipError_t launch_row_cdf(const float* w, const uint8_t* mask, long long n, double scale, unsigned long long* cdf,
                          unsigned long long* scratch, hipStream_t st);
hipError_t launch_sample_epoch(const ShuffleKeys& sk, const DrawKeys& dk, const unsigned long long* cdf, long long n,
                               long long m, long long bs, const float* coords, const float* gt, const float* dist,
                               const uint8_t* mask, float* coords_out, float* gt_out, float* dist_out, uint8_t* mask_out,
                               int* batch_counts, long long* order_out, hipStream_t st);

// rows of a coordinate grid (inr_grid.hip): the description of inr_grid_desc plus what the host derives
// from it -- the three steps (IEEE divisions) and the (k, y, x) of the chunk's first row
struct GridArgs {
  int coils_total, n_coils, H, W;
  float wy0, wy1, wx0, wx1;
  float step_z, step_y, step_x;
  unsigned k_lo, y_lo, x_lo;
  int coils[64];
};
hipError_t launch_grid_rows(const GridArgs& g, long long n_rows, float* coords, float* dist, hipStream_t st);

// radial band statistics (inr_bands.hip): the bounds travel as kernel arguments
constexpr int BAND_MAX = 64;          // INR_BAND_MAX
constexpr int BAND_FIELDS = 7;        // INR_BAND_FIELDS
constexpr int BAND_TILE_ROWS = 1024;  // INR_BAND_TILE_ROWS
struct BandArgs {
  int n_bands, mask_select;
  float lo[BAND_MAX], hi[BAND_MAX];
};
long long band_stats_scratch_doubles(long long n, int n_bands);
hipError_t launch_band_stats(const BandArgs& a, const float* dist, const float* gt, const float* pred,
                             const uint8_t* mask, long long n, double* stats, double* scratch, hipStream_t st);

// per-ring scaling (inr_ring_scale.hip): ring r is radii[r] <= dist < radii[r+1]; the table travels as
// kernel arguments like BandArgs
struct RingArgs {
  int n_rings;
  float radii[BAND_MAX + 1], divisors[BAND_MAX];
};
hipError_t launch_ring_scale(const RingArgs& a, const float* dist, const float* in, float* out, long long n,
                             hipStream_t st);

// continuous radial scaling (inr_radial_scale.hip): a piecewise-linear profile on n_knots uniform knots
// from r_lo, 1 / inv_step apart; `profile` is device memory, staged in LDS by every block
constexpr int RADIAL_KNOTS_MAX = 4096;  // INR_RADIAL_KNOTS_MAX
hipError_t launch_radial_scale(const float* dist, const float* in, float* out, long long n, const float* profile,
                               int n_knots, float r_lo, float inv_step, bool multiply, hipStream_t st);

// learned radial gain (inr_gain.hip): res = y exp(-s), the loss on res and its gradients to y and s in one
// pass; the no-grad product alone.  res may be nullptr in the first
hipError_t launch_gain_loss_grad(const LossDesc& ld, const float* y, const float* s, const float* gt, const uint8_t* mask,
                                 long long B, float* res, float* loss_out, float* dy, float* ds, hipStream_t st);
hipError_t launch_gain_apply(const float* y, const float* s, long long B, float* res, hipStream_t st);

// mixture of heads (inr_mix.hip): res = clamp(sum_k w_k y_k), the loss on res plus expert k's own loss on
// ring k, and the gradients to every y_k and to w in one pass; the no-grad mix alone.  The tables travel as kernel
// arguments; y[k] / dy[k] are expert k's [B,2] buffers (dy unused by the second).  res may be nullptr in the first
constexpr int MIX_MAX_HEADS = 8;  // INR_MIX_MAX_HEADS
constexpr int MIX_BLOCKS = 55;    // INR_MIX_BLOCKS: 9 terms x 55 ordered partials behind the 10 result words
constexpr int MIX_PARTIALS = 10;  // INR_MIX_PARTIALS
struct MixArgs {
  int n_heads, detach, clamp;
  float radii[MIX_MAX_HEADS + 1];      // ring k: radii[k] <= dist <= radii[k+1]
  float inv_count[MIX_MAX_HEADS + 1];  // the mixed term's 1 / rows, then each ring's (0: no row)
  const float* y[MIX_MAX_HEADS];
  float* dy[MIX_MAX_HEADS];
};
hipError_t launch_mix_loss_grad(const LossDesc& ld, const MixArgs& a, const float* w, const float* gt, const float* dist,
                                const uint8_t* mask, long long B, float* res, float* loss_out, float* dw, hipStream_t st);
hipError_t launch_mix_apply(const MixArgs& a, const float* w, long long B, float* res, hipStream_t st);

// SENSE-model fits (inr_sense.hip): coil images x_g = scale * S_g * I of an image network's and a
// sensitivity network's outputs, written at the ifftshift-ed pixel when `shift`, and the adjoint of that product
hipError_t launch_sense_apply(const float* img, const float* sens, int G, long long H, long long W, float scale, int shift,
                              float* x, hipStream_t st);
hipError_t launch_sense_grad(const float* img, const float* sens, const float* gx, int G, long long H, long long W,
                             float scale, int shift, float* dimg, float* dsens, hipStream_t st);

// SENSE fits on calibrated coil maps (inr_sense_calib.hip): low-resolution coil images of the windowed
// centre block kc [C,a,b,2] at Ho x Wo separable positions (phasor tables ey [a,Ho,2], ex [b,Wo,2] from the host), unit-RSS
// maps of them, and the image half of launch_sense_grad alone
constexpr int SENSE_CALIB_MAX = 64;  // INR_SENSE_CALIB_MAX: entries per axis of the centre block
hipError_t launch_sense_lowres(const float* kc, const float* ey, const float* ex, int C, int a, int b, long long Ho,
                               long long Wo, float* out, hipStream_t st);
hipError_t launch_sense_maps(const float* low, int C, long long P, float floor, float* maps, float* rss, hipStream_t st);
hipError_t launch_sense_adjoint(const float* sens, const float* gx, int G, long long H, long long W, float scale, int shift,
                                float* dimg, hipStream_t st);

// total-variation prior on the image of a SENSE fit (inr_image_tv.hip): weight * TV of img [H,W,2] into
// loss_out[0], weight * dTV/dimg written or added into dimg (nullptr: the value alone).  loss_out[IMAGE_TV_PARTIALS ...]
// holds one fp64 partial per block
constexpr int IMAGE_TV_THREADS = 256;
constexpr int IMAGE_TV_BLOCKS = 255;   // INR_IMAGE_TV_BLOCKS
constexpr int IMAGE_TV_PARTIALS = 2;   // INR_IMAGE_TV_PARTIALS: word of the first fp64 partial (8-byte aligned with loss_out)
hipError_t launch_image_tv_grad(const float* img, long long H, long long W, float weight, float eps, bool accumulate,
                                float* loss_out, float* dimg, hipStream_t st);

// focal frequency loss (inr_loss_focal.hip): the batch's largest weight, then the weighted squared error
// and its gradient; the words of loss_out are laid out by the FOCAL_* constants.  dout may be nullptr
constexpr int FOCAL_BLOCKS = 255;    // INR_FOCAL_BLOCKS
constexpr int FOCAL_PARTIALS = 1;    // INR_FOCAL_PARTIALS
constexpr int FOCAL_MAXIMA = 256;    // INR_FOCAL_MAXIMA
constexpr int FOCAL_NMAX = 511;      // INR_FOCAL_NMAX
struct FocalArgs {
  float alpha;
  int log_matrix;
  float loss_weight;  // as given; the kernel doubles it (exactly) for the gradient
  float inv_count;
};
hipError_t launch_focal_loss_grad(const FocalArgs& a, const float* out, const float* gt, const uint8_t* mask, long long B,
                                  float* loss_out, float* dout, hipStream_t st);

// coil compression (inr_coils.hip): Gram matrix of a coil-major scan, product with a small matrix
constexpr int COIL_MAX = 32;           // INR_COIL_MAX
constexpr int COIL_TILE_PIXELS = 128;  // INR_COIL_TILE_PIXELS
long long coil_gram_scratch_doubles(int C, long long N);
hipError_t launch_coil_gram(const float* data, int C, long long N, double* gram, double* scratch, hipStream_t st);
hipError_t launch_coil_apply(const float* in, const float* A, int M, int K, long long N, float* out, hipStream_t st);

// off-grid samples of the continuous k-space (inr_nudft.hip): phasor tables in scratch, then the
// contraction on the fp32 matrix pipe
constexpr int NUDFT_TILE = 64;  // INR_NUDFT_TILE: samples per workgroup
long long nudft_scratch_floats(long long H, long long W, long long M);
hipError_t launch_nudft(const float* img, int C, int H, int W, const double* pos, long long M, float* out,
                        float* scratch, hipStream_t st);

// the conjugate transpose of launch_nudft (inr_nudft_adjoint.hip): samples [C][M][2], optional weights
// [M] -> coil images [C][H][W][2], from the same tables
long long adjoint_nudft_scratch_floats(long long H, long long W, long long M);
hipError_t launch_adjoint_nudft(const float* val, const double* pos, const float* w, int C, int H, int W, long long M,
                                float* out, float* scratch, hipStream_t st);

// table-based (Kaiser-Bessel) gridding of the same two operators (inr_nufft.hip): oversampling 2, six
// taps per axis; the FFT between prepare and interp, and between spread and finish, is the caller's
constexpr int NUFFT_TAPS = 6;   // INR_NUFFT_TAPS
constexpr int NUFFT_TILE = 16;  // INR_NUFFT_TILE: grid cells per edge of a spread tile and of a bin
inline long long nufft_bin_count(long long H, long long W) {
  return ((2 * H + NUFFT_TILE - 1) / NUFFT_TILE) * ((2 * W + NUFFT_TILE - 1) / NUFFT_TILE);
}
long long nufft_scratch_floats(long long M);
hipError_t launch_nufft_prepare(const float* img, const float* apod_y, const float* apod_x, int C, int H, int W,
                                float* grid, hipStream_t st);
hipError_t launch_nufft_finish(const float* grid, const float* apod_y, const float* apod_x, int C, int H, int W,
                               float* out, hipStream_t st);
// `plain`: the grid is laid out as torch.fft reads and writes it -- the centred grid rolled by (H, W), so that cell
// (jy, jx) lives at ((jy + H) mod 2H, (jx + W) mod 2W) and no shifted copy surrounds the caller's FFT
hipError_t launch_nufft_interp(const float* grid, const double* pos, int C, int H, int W, long long M, bool plain,
                               float* out, float* scratch, hipStream_t st);
hipError_t launch_nufft_spread(const float* val, const double* pos, const float* w, const int* bin_start,
                               const int* order, int C, int H, int W, long long M, bool plain, float* grid, float* scratch,
                               hipStream_t st);
// 2 / (a_y a_x): one product, one division, the doubling exact
__device__ inline float deapodise(float ay, float ax) { return 2.0f / (ay * ax); }

// off-grid SENSE fits on calibrated maps (inr_sense_nufft.hip): launch_sense_apply(shift 0) fused with
// launch_nufft_prepare, and launch_nufft_finish fused with launch_sense_adjoint(shift 0), both on the plain-layout grid
hipError_t launch_sense_nufft_prepare(const float* img, const float* maps, const float* apod_y, const float* apod_x, int G,
                                      int H, int W, float scale, float* grid, hipStream_t st);
hipError_t launch_sense_nufft_finish(const float* grid, const float* maps, const float* apod_y, const float* apod_x, int G,
                                     int H, int W, float scale, float* dimg, bool accumulate, hipStream_t st);

}  // namespace inr
