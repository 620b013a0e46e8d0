// inr_api_aux.hip -- the entries of the C-ABI (include/inr_abi.h) that launch no network, the off-grid operators apart
// (inr_api_offgrid.hip): encoders, losses, TV, Adam, image metrics, display, shuffle, weighted epochs, grid rows, band
// statistics, per-ring and continuous radial scaling, learned radial gain, mixture of heads, the SENSE product, its calibrated-map entries and the TV prior on its image, focal frequency loss, coil compression.  Each checks its arguments, fills an argument struct, launches and maps
// the hipError_t to a code; none allocates device memory or syncs.
#include <cmath>
#include <cstring>

#include "inr_host.h"

void to_loss_desc(const inr_loss_desc* l, LossDesc* o) {
  memset(o, 0, sizeof(*o));
  o->scale = l->scale == 0.f ? 1.f : l->scale;
  o->cons_w = l->cons_w;
  o->cons_chan = l->cons_chan == 1 ? 1 : 2;
  for (int i = 0; i < INR_MAX_HEADS; ++i) {
    o->cons_lo[i] = l->cons_lo[i];
    o->cons_hi[i] = l->cons_hi[i];
    o->cons_inv[i] = l->cons_inv[i];
  }
  o->kind = l->kind;
  o->eps = l->eps;
  o->sigma = l->sigma;
  o->factor = l->factor;
  o->inv_count = l->inv_count;
  o->hdr_A = l->hdr_A;
}

static bool has_complex_tensors(const NetDesc& nd) {
  for (int l = 0; l < nd.ND; ++l)
    if (nd.L[l].ltype == LT_WIRE_HIDDEN || nd.L[l].ltype == LT_WIRE_LAST) return true;
  return false;
}

// the Adam kernels form the penalty gradients per REAL entry: right for every tensor of a real model, wrong for complex64
int check_real_penalty(const inr_plan* plan, double l1, double l2, const char* who) {
  if ((l1 != 0.0 || l2 != 0.0) && has_complex_tensors(plan->nd))
    return fail(INR_ERR_INVALID, "%s: l1 / l2 on a plan with complex64 tensors -- add the penalty gradient with "
                "inr_reg_grad and pass l1 = l2 = 0", who);
  return INR_OK;
}

// torch computes these in Python doubles and passes them to fp32 kernels as scalars
void adam_bias_terms(double lr, double beta1, double beta2, int32_t step, float* step_size, float* bc2_sqrt) {
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  *step_size = (float)(lr / bc1);
  *bc2_sqrt = (float)std::sqrt(bc2);
}

// AdamArgs of an update from the doubles of its ABI call; (step_size, bc2_sqrt) are the caller's: adam_bias_terms, or a
// device-resident schedule
inr::AdamArgs adam_args(double beta1, double beta2, double eps, double weight_decay, double l1, double l2) {
  inr::AdamArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.do_update = 1;
  aa.step_size = 0.f;
  aa.bc2_sqrt = 1.f;
  aa.omb1 = (float)(1.0 - beta1);
  aa.beta2 = (float)beta2;
  aa.omb2 = (float)(1.0 - beta2);
  aa.eps = (float)eps;
  aa.weight_decay = (float)weight_decay;
  aa.l1 = (float)l1;
  aa.l2 = (float)l2;
  return aa;
}

int coil_count_check(int32_t v, const char* name, const char* who) {
  if (v < 1 || v > INR_COIL_MAX) return fail(INR_ERR_INVALID, "%s: %s = %d (1..%d)", who, name, (int)v, INR_COIL_MAX);
  return INR_OK;
}

bool ranges_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

extern "C" {

int inr_pack_params(const inr_plan* plan, const float* params, float* packed, void* stream) {
  if (plan == nullptr || params == nullptr || packed == nullptr)
    return fail(INR_ERR_INVALID, "inr_pack_params: null argument");
  inr::AdamArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.do_update = 0;
  hipError_t e = inr::launch_adam_pack(plan->nd, const_cast<float*>(params), nullptr, nullptr, nullptr, packed, aa,
                                       (hipStream_t)stream);
  if (e == hipSuccess) images_note(plan, IMG_EV_PACK, inr::IMG_ALL, (hipStream_t)stream);
  return hip_done(e, "inr_pack_params");
}

int inr_encode_logf(const float* coords, const float* bands, int64_t B, int32_t n_bands, float* out, void* stream) {
  if (coords == nullptr || bands == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_encode_logf: null argument");
  if (B <= 0 || n_bands <= 0) return fail(INR_ERR_INVALID, "inr_encode_logf: B %lld, n_bands %d", (long long)B, n_bands);
  hipError_t e = inr::launch_encode_logf(coords, bands, B, n_bands, out, (hipStream_t)stream);
  return hip_done(e, "inr_encode_logf");
}

int inr_encode_gauss(const float* coords, const float* enc_B, int64_t B, int32_t E, float* out, void* stream) {
  if (coords == nullptr || enc_B == nullptr || out == nullptr)
    return fail(INR_ERR_INVALID, "inr_encode_gauss: null argument");
  if (B <= 0 || E <= 0) return fail(INR_ERR_INVALID, "inr_encode_gauss: B = %lld, E = %d", (long long)B, E);
  hipError_t e = inr::launch_encode_gauss(coords, enc_B, B, E, out, (hipStream_t)stream);
  return hip_done(e, "inr_encode_gauss");
}

int inr_loss_grad(const inr_loss_desc* loss, const float* out, const float* gt, const float* kcoords,
                  const uint8_t* mask, int64_t B, float* loss_out, float* dout, void* stream) {
  if (loss == nullptr || out == nullptr || gt == nullptr || loss_out == nullptr || dout == nullptr)
    return fail(INR_ERR_INVALID, "inr_loss_grad: null argument");
  if (loss->kind < INR_LOSS_L2_HALF || loss->kind > INR_LOSS_CENTER)
    return fail(INR_ERR_INVALID, "inr_loss_grad: loss kind %d", loss->kind);
  if (B <= 0) return fail(INR_ERR_INVALID, "inr_loss_grad: B = %lld", (long long)B);
  LossDesc ld;
  to_loss_desc(loss, &ld);
  hipError_t e = inr::launch_loss_grad(ld, out, gt, mask, B, loss_out, dout, (hipStream_t)stream);
  return hip_done(e, "inr_loss_grad");
}

int inr_loss_grad_multi(const inr_loss_desc* loss, const float* outs, const float* gt, const float* dist,
                        const uint8_t* mask, int32_t n_heads, int64_t B, float* loss_out, float* douts, void* stream) {
  if (loss == nullptr || outs == nullptr || gt == nullptr || loss_out == nullptr || douts == nullptr)
    return fail(INR_ERR_INVALID, "inr_loss_grad_multi: null argument");
  if (loss->kind < INR_LOSS_L2_HALF || loss->kind > INR_LOSS_CENTER)
    return fail(INR_ERR_INVALID, "inr_loss_grad_multi: loss kind %d", loss->kind);
  if (n_heads < 1 || n_heads > INR_MAX_HEADS || B <= 0)
    return fail(INR_ERR_INVALID, "inr_loss_grad_multi: n_heads %d, B %lld", n_heads, (long long)B);
  if (loss->cons_w != 0.f && dist == nullptr)
    return fail(INR_ERR_INVALID, "inr_loss_grad_multi: the consistency term needs dist");
  LossDesc ld;
  to_loss_desc(loss, &ld);
  hipError_t e = inr::launch_loss_grad_multi(ld, outs, gt, dist, mask, n_heads, B, loss_out, douts, (hipStream_t)stream);
  return hip_done(e, "inr_loss_grad_multi");
}

// weights of the TV term's horizontal and vertical differences of a W x H image
static void tv_coeffs(float weight, int64_t W, int64_t H, float* cw, float* ch) {
  *cw = (float)((double)weight / ((double)H * (double)(W - 1) * 2.0));
  *ch = (float)((double)weight / ((double)(H - 1) * (double)W * 2.0));
}

int inr_tv_grad(const float* out, int64_t R, int64_t R_own, int64_t W, int64_t H, float weight,
                float* loss_out, float* dout, void* stream) {
  if (out == nullptr || loss_out == nullptr || dout == nullptr) return fail(INR_ERR_INVALID, "inr_tv_grad: null argument");
  if (R <= 0 || R_own <= 0 || R_own > R || R > R_own + 1 || W < 2 || H < 2 || R > H)
    return fail(INR_ERR_INVALID, "inr_tv_grad: R %lld R_own %lld W %lld H %lld", (long long)R, (long long)R_own,
                (long long)W, (long long)H);
  float cw, ch;
  tv_coeffs(weight, W, H, &cw, &ch);
  hipError_t e = inr::launch_tv_grad(out, R, R_own, W, cw, ch, loss_out, dout, (hipStream_t)stream);
  return hip_done(e, "inr_tv_grad");
}

int inr_loss_tv_grad(const inr_loss_desc* loss, const float* out, const float* gt, const uint8_t* mask, int64_t R,
                     int64_t R_own, int64_t W, int64_t H, float tv_weight, float* loss_out, float* dout, void* stream) {
  if (loss == nullptr || out == nullptr || gt == nullptr || loss_out == nullptr || dout == nullptr)
    return fail(INR_ERR_INVALID, "inr_loss_tv_grad: null argument");
  if (loss->kind < INR_LOSS_L2_HALF || loss->kind > INR_LOSS_CENTER)
    return fail(INR_ERR_INVALID, "inr_loss_tv_grad: loss kind %d", loss->kind);
  if (R <= 0 || R_own <= 0 || R_own > R || R > R_own + 1 || W < 2 || H < 2 || R > H)
    return fail(INR_ERR_INVALID, "inr_loss_tv_grad: R %lld R_own %lld W %lld H %lld", (long long)R, (long long)R_own,
                (long long)W, (long long)H);
  LossDesc ld;
  to_loss_desc(loss, &ld);
  float cw, ch;
  tv_coeffs(tv_weight, W, H, &cw, &ch);
  hipError_t e = inr::launch_loss_tv_grad(ld, out, gt, mask, R, R_own, W, cw, ch, loss_out, dout, (hipStream_t)stream);
  return hip_done(e, "inr_loss_tv_grad");
}

int inr_center_pairs_grad(const float* out, const float* gt, const int64_t* idx_a, const int64_t* idx_b, int64_t n,
                          int64_t B, float weight, float* loss_out, float* dout, void* stream) {
  if (out == nullptr || gt == nullptr || idx_a == nullptr || idx_b == nullptr || loss_out == nullptr || dout == nullptr)
    return fail(INR_ERR_INVALID, "inr_center_pairs_grad: null argument");
  if (n <= 0 || B <= 0) return fail(INR_ERR_INVALID, "inr_center_pairs_grad: n %lld B %lld", (long long)n, (long long)B);
  hipError_t e = inr::launch_center_pairs(out, gt, (const long long*)idx_a, (const long long*)idx_b, n, B,
                                          (float)((double)weight / (double)n), loss_out, dout, (hipStream_t)stream);
  return hip_done(e, "inr_center_pairs_grad");
}

static int image_metrics_check(int64_t C, int64_t H, int64_t W, const char* who) {
  if (C < 1 || H < 1 || W < 1 || C > (1LL << 30) || H > (1LL << 30) || W > (1LL << 30) || C * H * W > (1LL << 40))
    return fail(INR_ERR_INVALID, "%s: C %lld, H %lld, W %lld", who, (long long)C, (long long)H, (long long)W);
  return INR_OK;
}

int inr_image_metrics_scratch(int64_t C, int64_t H, int64_t W, int64_t* scratch_doubles) {
  if (scratch_doubles == nullptr) return fail(INR_ERR_INVALID, "inr_image_metrics_scratch: null argument");
  const int rc = image_metrics_check(C, H, W, "inr_image_metrics_scratch");
  if (rc != INR_OK) return rc;
  *scratch_doubles = inr::image_metrics_scratch_doubles(H, W);
  return INR_OK;
}

int inr_image_metrics(const float* coils, int64_t C, int64_t H, int64_t W, const float* ref, float* rss_out,
                      double* metrics_out, double* scratch, int64_t scratch_doubles, void* stream) {
  if (coils == nullptr || rss_out == nullptr) return fail(INR_ERR_INVALID, "inr_image_metrics: null argument");
  const int rc = image_metrics_check(C, H, W, "inr_image_metrics");
  if (rc != INR_OK) return rc;
  if (ref != nullptr) {
    if (metrics_out == nullptr || scratch == nullptr)
      return fail(INR_ERR_INVALID, "inr_image_metrics: a reference image needs metrics_out and scratch");
    if (H < 7 || W < 7)  // skimage.metrics.structural_similarity raises the same way
      return fail(INR_ERR_INVALID, "inr_image_metrics: win_size exceeds image extent (SSIM needs H, W >= 7; got %lld x %lld)",
                  (long long)H, (long long)W);
    const long long need = inr::image_metrics_scratch_doubles(H, W);
    if (scratch_doubles < need)
      return fail(INR_ERR_INVALID, "inr_image_metrics: scratch holds %lld doubles, needs %lld", (long long)scratch_doubles,
                  need);
  }
  hipError_t e = inr::launch_image_metrics(coils, (int)C, (int)H, (int)W, ref, rss_out, metrics_out, scratch,
                                           (hipStream_t)stream);
  return hip_done(e, "inr_image_metrics");
}

// ---- pictures and per-coil table of the validation epoch (inr_display.hip) ----
int inr_kspace_display_scratch(int64_t C, int64_t H, int64_t W, int64_t* scratch_floats) {
  if (scratch_floats == nullptr) return fail(INR_ERR_INVALID, "inr_kspace_display_scratch: null argument");
  const int rc = image_metrics_check(C, H, W, "inr_kspace_display_scratch");
  if (rc != INR_OK) return rc;
  *scratch_floats = inr::kspace_display_scratch_floats(H, W);
  return INR_OK;
}

int inr_kspace_display(const float* coils, const float* minus, int64_t C, int64_t H, int64_t W, float smoothing_factor,
                       float* out, float* scratch, int64_t scratch_floats, void* stream) {
  if (coils == nullptr || out == nullptr || scratch == nullptr)
    return fail(INR_ERR_INVALID, "inr_kspace_display: null argument");
  const int rc = image_metrics_check(C, H, W, "inr_kspace_display");
  if (rc != INR_OK) return rc;
  if (((uintptr_t)coils | (uintptr_t)minus) & 7u)
    return fail(INR_ERR_INVALID, "inr_kspace_display: coils / minus must be 8-byte aligned ((re, im) pairs move as one load)");
  if (!(smoothing_factor == smoothing_factor))
    return fail(INR_ERR_INVALID, "inr_kspace_display: smoothing_factor is NaN");
  const long long need = inr::kspace_display_scratch_floats(H, W);
  if (scratch_floats < need)
    return fail(INR_ERR_INVALID, "inr_kspace_display: scratch holds %lld floats, needs %lld", (long long)scratch_floats, need);
  // torch.expm1 of the fp32 scalar (models/utils.py:264-265): evaluated in double here and rounded once
  const float em = (float)std::expm1((double)smoothing_factor);
  hipError_t e = inr::launch_kspace_display(coils, minus, (int)C, (int)H, (int)W, em, out, scratch, (hipStream_t)stream);
  return hip_done(e, "inr_kspace_display");
}

int inr_gray8_scratch(int64_t H, int64_t W, int64_t* scratch_floats) {
  if (scratch_floats == nullptr) return fail(INR_ERR_INVALID, "inr_gray8_scratch: null argument");
  const int rc = image_metrics_check(1, H, W, "inr_gray8_scratch");
  if (rc != INR_OK) return rc;
  *scratch_floats = inr::gray8_scratch_floats(H, W);
  return INR_OK;
}

int inr_gray8(const float* img, int64_t H, int64_t W, int32_t take_abs, int32_t has_range, float vmin, float vmax,
              const uint8_t* lut, uint8_t* out, float* norm_out, float* scratch, int64_t scratch_floats, void* stream) {
  if (img == nullptr || lut == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_gray8: null argument");
  const int rc = image_metrics_check(1, H, W, "inr_gray8");
  if (rc != INR_OK) return rc;
  if (has_range) {
    if (!(vmin <= vmax))  // matplotlib.colors.Normalize raises the same way
      return fail(INR_ERR_INVALID, "inr_gray8: minvalue must be less than or equal to maxvalue (vmin %g, vmax %g)",
                  (double)vmin, (double)vmax);
  } else {
    const long long need = inr::gray8_scratch_floats(H, W);
    if (scratch == nullptr || scratch_floats < need)
      return fail(INR_ERR_INVALID, "inr_gray8: scratch holds %lld floats, needs %lld",
                  scratch == nullptr ? 0LL : (long long)scratch_floats, need);
  }
  hipError_t e = inr::launch_gray8(img, (int)H, (int)W, take_abs != 0, has_range != 0, vmin, vmax, lut, out, norm_out,
                                   scratch, (hipStream_t)stream);
  return hip_done(e, "inr_gray8");
}

static int coil_stats_check(int64_t C, int64_t H, int64_t W, const char* who) {
  const int rc = image_metrics_check(C, H, W, who);
  if (rc != INR_OK) return rc;
  if (C > 65535) return fail(INR_ERR_INVALID, "%s: C %lld (one grid row per coil: at most 65535)", who, (long long)C);
  return INR_OK;
}

int inr_coil_stats_scratch(int64_t C, int64_t H, int64_t W, int64_t* scratch_doubles) {
  if (scratch_doubles == nullptr) return fail(INR_ERR_INVALID, "inr_coil_stats_scratch: null argument");
  const int rc = coil_stats_check(C, H, W, "inr_coil_stats_scratch");
  if (rc != INR_OK) return rc;
  *scratch_doubles = inr::coil_stats_scratch_doubles(C, H, W);
  return INR_OK;
}

int inr_coil_stats(const float* coils, int64_t C, int64_t H, int64_t W, double* stats, double* scratch,
                   int64_t scratch_doubles, void* stream) {
  if (coils == nullptr || stats == nullptr || scratch == nullptr)
    return fail(INR_ERR_INVALID, "inr_coil_stats: null argument");
  const int rc = coil_stats_check(C, H, W, "inr_coil_stats");
  if (rc != INR_OK) return rc;
  if ((uintptr_t)coils & 7u)
    return fail(INR_ERR_INVALID, "inr_coil_stats: coils must be 8-byte aligned ((re, im) pairs move as one load)");
  const long long need = inr::coil_stats_scratch_doubles(C, H, W);
  if (scratch_doubles < need)
    return fail(INR_ERR_INVALID, "inr_coil_stats: scratch holds %lld doubles, needs %lld", (long long)scratch_doubles, need);
  hipError_t e = inr::launch_coil_stats(coils, (int)C, (int)H, (int)W, stats, scratch, (hipStream_t)stream);
  return hip_done(e, "inr_coil_stats");
}

// key schedule of the epoch permutation (inr_mi355x/shuffle.py round_keys is the same text in Python)
static inr::ShuffleKeys shuffle_keys(int64_t n, uint64_t seed, uint32_t epoch) {
  const uint32_t gold = 0x9E3779B9u;
  inr::ShuffleKeys sk;
  using inr::shuffle_mix;
  const uint32_t base = shuffle_mix(shuffle_mix(shuffle_mix((uint32_t)seed + gold) ^ (uint32_t)(seed >> 32)) + epoch);
  for (int r = 0; r < SHUFFLE_ROUNDS; ++r) sk.k[r] = shuffle_mix(base + (uint32_t)(r + 1) * gold);
  int k = 8;  // smallest even k >= 8 with 2^k >= n
  while ((1LL << k) < n) k += 2;
  sk.h = k / 2;
  return sk;
}

// the optional pairs of an epoch call (inr_shuffle_epoch, inr_sample_epoch) and its batch size
static int epoch_buffers_check(const char* who, int64_t batch_size, const float* coords, const float* gt, const float* dist,
                               const uint8_t* mask, const float* coords_out, const float* gt_out, const float* dist_out,
                               const uint8_t* mask_out, const int32_t* batch_counts, const int64_t* order_out) {
  if ((coords == nullptr) != (coords_out == nullptr) || (gt == nullptr) != (gt_out == nullptr) ||
      (dist == nullptr) != (dist_out == nullptr) || (mask == nullptr && mask_out != nullptr))
    return fail(INR_ERR_INVALID, "%s: an input and its output buffer go together", who);
  if (coords_out == nullptr && gt_out == nullptr && dist_out == nullptr && mask_out == nullptr &&
      batch_counts == nullptr && order_out == nullptr)
    return fail(INR_ERR_INVALID, "%s: no output", who);
  if (batch_counts != nullptr && (batch_size < 1 || batch_size >= (1LL << 31)))
    return fail(INR_ERR_INVALID, "%s: batch_counts with batch_size = %lld", who, (long long)batch_size);
  if (((uintptr_t)gt | (uintptr_t)gt_out) & 7u)
    return fail(INR_ERR_INVALID, "%s: gt / gt_out must be 8-byte aligned ([n,2] rows move as one load)", who);
  if ((coords != nullptr && coords == coords_out) || (gt != nullptr && gt == gt_out) ||
      (dist != nullptr && dist == dist_out) || (mask != nullptr && mask == mask_out))
    return fail(INR_ERR_INVALID, "%s: in-place (an output buffer is its input)", who);
  return INR_OK;
}

int inr_shuffle_epoch(int64_t n, int64_t batch_size, uint64_t seed, uint32_t epoch, const float* coords,
                      const float* gt, const float* dist, const uint8_t* mask, float* coords_out, float* gt_out,
                      float* dist_out, uint8_t* mask_out, int32_t* batch_counts, int64_t* order_out, void* stream) {
  if (n < 1 || n >= (1LL << 31))
    return fail(INR_ERR_INVALID, "inr_shuffle_epoch: n = %lld (the 32-bit permutation covers 1 <= n < 2^31)", (long long)n);
  if (int rc = epoch_buffers_check("inr_shuffle_epoch", batch_size, coords, gt, dist, mask, coords_out, gt_out, dist_out,
                                   mask_out, batch_counts, order_out))
    return rc;
  const inr::ShuffleKeys sk = shuffle_keys(n, seed, epoch);
  hipError_t e = inr::launch_shuffle_epoch(sk, n, batch_size, coords, gt, dist, mask, coords_out, gt_out, dist_out,
                                           mask_out, batch_counts, (long long*)order_out, (hipStream_t)stream);
  return hip_done(e, "inr_shuffle_epoch");
}

// ---- weighted epochs (inr_sample.hip) ----
// keys of a stratum's offset: the schedule of shuffle_keys with another constant, so that the offsets share nothing with
// the permutation of the same (seed, epoch) (inr_mi355x/sampling.py draw_keys is the same text in Python)
static inr::DrawKeys draw_keys(uint64_t seed, uint32_t epoch) {
  const uint32_t c = 0x85EBCA6Bu;
  using inr::shuffle_mix;
  const uint32_t base = shuffle_mix(shuffle_mix(shuffle_mix((uint32_t)seed + c) ^ (uint32_t)(seed >> 32)) + epoch);
  inr::DrawKeys dk;
  for (int r = 0; r < 2; ++r) dk.k[r] = shuffle_mix(base + (uint32_t)(r + 1) * c);
  return dk;
}

static int row_count_check(const char* who, const char* name, int64_t v) {
  if (v < 1 || v >= (1LL << 31)) return fail(INR_ERR_INVALID, "%s: %s = %lld (1 <= %s < 2^31)", who, name, (long long)v, name);
  return INR_OK;
}

int inr_row_cdf_scratch(int64_t n, int64_t* scratch_words) {
  if (scratch_words == nullptr) return fail(INR_ERR_INVALID, "inr_row_cdf_scratch: null argument");
  if (int rc = row_count_check("inr_row_cdf_scratch", "n", n)) return rc;
  *scratch_words = inr::row_cdf_scratch_words(n);
  return INR_OK;
}

int inr_row_cdf(const float* w, const uint8_t* mask, int64_t n, double scale, uint64_t* cdf_out, uint64_t* scratch,
                int64_t scratch_words, void* stream) {
  if (w == nullptr || cdf_out == nullptr || scratch == nullptr) return fail(INR_ERR_INVALID, "inr_row_cdf: null argument");
  if (int rc = row_count_check("inr_row_cdf", "n", n)) return rc;
  if (!std::isfinite(scale) || scale <= 0.0)
    return fail(INR_ERR_INVALID, "inr_row_cdf: scale = %g (must be finite and > 0)", scale);
  if (((uintptr_t)w & 3u) != 0 || (((uintptr_t)cdf_out | (uintptr_t)scratch) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_row_cdf: w must be 4-byte aligned, cdf_out and scratch 8-byte aligned");
  const int64_t need = inr::row_cdf_scratch_words(n);
  if (scratch_words < need)
    return fail(INR_ERR_INVALID, "inr_row_cdf: scratch holds %lld words, needs %lld", (long long)scratch_words, (long long)need);
  if (ranges_overlap(cdf_out, n * 8, w, n * 4) || ranges_overlap(cdf_out, n * 8, scratch, need * 8) ||
      ranges_overlap(scratch, need * 8, w, n * 4) ||
      (mask != nullptr && (ranges_overlap(cdf_out, n * 8, mask, n) || ranges_overlap(scratch, need * 8, mask, n))))
    return fail(INR_ERR_INVALID, "inr_row_cdf: cdf_out / scratch overlaps another buffer");
  hipError_t e = inr::launch_row_cdf(w, mask, n, scale, (unsigned long long*)cdf_out, (unsigned long long*)scratch,
                                     (hipStream_t)stream);
  return hip_done(e, "inr_row_cdf");
}

int inr_sample_epoch(const uint64_t* cdf, int64_t n, int64_t m, int64_t batch_size, uint64_t seed, uint32_t epoch,
                     const float* coords, const float* gt, const float* dist, const uint8_t* mask, float* coords_out,
                     float* gt_out, float* dist_out, uint8_t* mask_out, int32_t* batch_counts, int64_t* order_out,
                     void* stream) {
  if (cdf == nullptr) return fail(INR_ERR_INVALID, "inr_sample_epoch: null argument");
  if (((uintptr_t)cdf & 7u) != 0) return fail(INR_ERR_INVALID, "inr_sample_epoch: cdf is not 8-byte aligned");
  if (int rc = row_count_check("inr_sample_epoch", "n", n)) return rc;
  if (int rc = row_count_check("inr_sample_epoch", "m", m)) return rc;
  if (int rc = epoch_buffers_check("inr_sample_epoch", batch_size, coords, gt, dist, mask, coords_out, gt_out, dist_out,
                                   mask_out, batch_counts, order_out))
    return rc;
  const inr::ShuffleKeys sk = shuffle_keys(m, seed, epoch);  // the strata are permuted, not the rows
  hipError_t e = inr::launch_sample_epoch(sk, draw_keys(seed, epoch), (const unsigned long long*)cdf, n, m, batch_size,
                                          coords, gt, dist, mask, coords_out, gt_out, dist_out, mask_out, batch_counts,
                                          (long long*)order_out, (hipStream_t)stream);
  return hip_done(e, "inr_sample_epoch");
}

// ---- rows of a coordinate grid (inr_grid.hip) ----
// step of an axis of n points over [a, b]: one fp32 subtraction and one fp32 division (IEEE on the host)
static float grid_step(float a, float b, int32_t n) {
  if (n == 1) return 0.f;
  const float span = b - a;
  return span / (float)(n - 1);
}

int inr_grid_rows(const inr_grid_desc* g, int64_t row_lo, int64_t n_rows, float* coords, float* dist, void* stream) {
  if (g == nullptr || coords == nullptr) return fail(INR_ERR_INVALID, "inr_grid_rows: null argument");
  if (g->H < 1 || g->W < 1 || g->n_coils < 1 || g->coils_total < 1)
    return fail(INR_ERR_INVALID, "inr_grid_rows: H = %d, W = %d, n_coils = %d, coils_total = %d (each must be >= 1)",
                (int)g->H, (int)g->W, (int)g->n_coils, (int)g->coils_total);
  if (g->n_coils > 64) return fail(INR_ERR_INVALID, "inr_grid_rows: n_coils = %d (at most 64 per call)", (int)g->n_coils);
  for (int k = 0; k < g->n_coils; ++k)
    if (g->coils[k] < 0 || g->coils[k] >= g->coils_total)
      return fail(INR_ERR_INVALID, "inr_grid_rows: coils[%d] = %d is outside [0, %d)", k, (int)g->coils[k],
                  (int)g->coils_total);
  if (!std::isfinite(g->y0) || !std::isfinite(g->y1) || !std::isfinite(g->x0) || !std::isfinite(g->x1))
    return fail(INR_ERR_INVALID, "inr_grid_rows: non-finite window (%g, %g, %g, %g)", (double)g->y0, (double)g->y1,
                (double)g->x0, (double)g->x1);
  const long long plane = (long long)g->H * g->W;  // < 2^62; 64 planes may not fit
  if (plane > INT64_MAX / g->n_coils)
    return fail(INR_ERR_INVALID, "inr_grid_rows: %d x %d x %d rows do not fit in 63 bits", (int)g->n_coils, (int)g->H, (int)g->W);
  const long long total = plane * g->n_coils;
  if (row_lo < 0 || n_rows < 0 || n_rows >= (1LL << 31) || row_lo > total || n_rows > total - row_lo)
    return fail(INR_ERR_INVALID, "inr_grid_rows: rows [%lld, %lld + %lld) of a grid of %lld (0 <= n_rows < 2^31 per call)",
                (long long)row_lo, (long long)row_lo, (long long)n_rows, total);
  if (n_rows == 0) return INR_OK;
  inr::GridArgs a;
  a.coils_total = g->coils_total;
  a.n_coils = g->n_coils;
  a.H = g->H;
  a.W = g->W;
  a.wy0 = g->y0;
  a.wy1 = g->y1;
  a.wx0 = g->x0;
  a.wx1 = g->x1;
  a.step_z = grid_step(-1.f, 1.f, g->coils_total);
  a.step_y = grid_step(g->y0, g->y1, g->H);
  a.step_x = grid_step(g->x0, g->x1, g->W);
  a.x_lo = (unsigned)(row_lo % g->W);
  a.y_lo = (unsigned)((row_lo / g->W) % g->H);
  a.k_lo = (unsigned)(row_lo / plane);
  for (int k = 0; k < 64; ++k) a.coils[k] = k < g->n_coils ? g->coils[k] : 0;
  hipError_t e = inr::launch_grid_rows(a, n_rows, coords, dist, (hipStream_t)stream);
  return hip_done(e, "inr_grid_rows");
}

// ---- radial band statistics (inr_bands.hip) ----
static_assert(INR_BAND_MAX == inr::BAND_MAX && INR_BAND_FIELDS == inr::BAND_FIELDS &&
                  INR_BAND_TILE_ROWS == inr::BAND_TILE_ROWS, "inr_abi.h and inr_aux.h disagree");

static int band_stats_check(int64_t n, int32_t n_bands, const char* who) {
  if (n < 1 || n >= (1LL << 31)) return fail(INR_ERR_INVALID, "%s: n = %lld (1 <= n < 2^31 rows per call)", who, (long long)n);
  if (n_bands < 1 || n_bands > INR_BAND_MAX)
    return fail(INR_ERR_INVALID, "%s: n_bands = %d (1..%d)", who, (int)n_bands, INR_BAND_MAX);
  return INR_OK;
}

int inr_band_stats_scratch(int64_t n, int32_t n_bands, int64_t* scratch_doubles) {
  if (scratch_doubles == nullptr) return fail(INR_ERR_INVALID, "inr_band_stats_scratch: null argument");
  const int rc = band_stats_check(n, n_bands, "inr_band_stats_scratch");
  if (rc != INR_OK) return rc;
  *scratch_doubles = inr::band_stats_scratch_doubles(n, n_bands);
  return INR_OK;
}

int inr_band_stats(const float* dist, const float* gt, const float* pred, const uint8_t* mask, int32_t mask_select,
                   int64_t n, const float* band_lo, const float* band_hi, int32_t n_bands, double* stats,
                   double* scratch, void* stream) {
  if (dist == nullptr || gt == nullptr || band_lo == nullptr || band_hi == nullptr || stats == nullptr || scratch == nullptr)
    return fail(INR_ERR_INVALID, "inr_band_stats: null argument");
  const int rc = band_stats_check(n, n_bands, "inr_band_stats");
  if (rc != INR_OK) return rc;
  inr::BandArgs a;
  a.n_bands = n_bands;
  a.mask_select = mask_select != 0;
  for (int b = 0; b < INR_BAND_MAX; ++b) {
    if (b < n_bands && !(band_lo[b] <= band_hi[b]))  // NaN bounds too
      return fail(INR_ERR_INVALID, "inr_band_stats: band %d is [%g, %g] (bounds must be numbers with lo <= hi)", b,
                  (double)band_lo[b], (double)band_hi[b]);
    a.lo[b] = b < n_bands ? band_lo[b] : 0.f;
    a.hi[b] = b < n_bands ? band_hi[b] : 0.f;
  }
  hipError_t e = inr::launch_band_stats(a, dist, gt, pred, mask, n, stats, scratch, (hipStream_t)stream);
  return hip_done(e, "inr_band_stats");
}

// ---- per-ring scaling (inr_ring_scale.hip) and continuous radial scaling (inr_radial_scale.hip; 4.24) ----
// the checks the two entries share: the row count, and where dist [n], in [n,2] and out [n,2] lie
static int scale_rows_count_check(int64_t n, const char* who) {
  if (n < 1 || n >= (1LL << 31)) return fail(INR_ERR_INVALID, "%s: n = %lld (1 <= n < 2^31 rows per call)", who, (long long)n);
  return INR_OK;
}

static int scale_rows_layout_check(const float* dist, const float* in, const float* out, int64_t n, const char* who) {
  if ((((uintptr_t)in | (uintptr_t)out) & 7u) != 0 || ((uintptr_t)dist & 3u) != 0)
    return fail(INR_ERR_INVALID, "%s: in / out must be 8-byte aligned and dist 4-byte aligned", who);
  if (out != in && ranges_overlap(out, n * 8, in, n * 8))
    return fail(INR_ERR_INVALID, "%s: out overlaps in partially (in place means out == in)", who);
  if (ranges_overlap(out, n * 8, dist, n * 4)) return fail(INR_ERR_INVALID, "%s: out overlaps dist", who);
  return INR_OK;
}

int inr_ring_scale(const float* dist, const float* in, float* out, int64_t n, const float* radii, const float* divisors,
                   int32_t n_rings, void* stream) {
  if (dist == nullptr || in == nullptr || out == nullptr || radii == nullptr || divisors == nullptr)
    return fail(INR_ERR_INVALID, "inr_ring_scale: null argument");
  if (int rc = scale_rows_count_check(n, "inr_ring_scale")) return rc;
  if (n_rings < 1 || n_rings > INR_BAND_MAX)
    return fail(INR_ERR_INVALID, "inr_ring_scale: n_rings = %d (1..%d)", (int)n_rings, INR_BAND_MAX);
  inr::RingArgs a;
  memset(&a, 0, sizeof(a));
  a.n_rings = n_rings;
  for (int r = 0; r <= n_rings; ++r) {
    if (!(radii[r] == radii[r])) return fail(INR_ERR_INVALID, "inr_ring_scale: radii[%d] is NaN", r);
    if (r > 0 && radii[r] < radii[r - 1])
      return fail(INR_ERR_INVALID, "inr_ring_scale: radii[%d] = %g is below radii[%d] = %g (radii must not decrease)", r,
                  (double)radii[r], r - 1, (double)radii[r - 1]);
    a.radii[r] = radii[r];
  }
  for (int r = 0; r < n_rings; ++r) {
    if (!std::isfinite(divisors[r]) || divisors[r] == 0.f)
      return fail(INR_ERR_INVALID, "inr_ring_scale: divisors[%d] = %g (must be finite and not zero)", r, (double)divisors[r]);
    a.divisors[r] = divisors[r];
  }
  if (int rc = scale_rows_layout_check(dist, in, out, n, "inr_ring_scale")) return rc;
  hipError_t e = inr::launch_ring_scale(a, dist, in, out, n, (hipStream_t)stream);
  return hip_done(e, "inr_ring_scale");
}

static_assert(INR_RADIAL_KNOTS_MAX == inr::RADIAL_KNOTS_MAX, "inr_abi.h and inr_aux.h disagree");

int inr_radial_scale(const float* dist, const float* in, float* out, int64_t n, const float* profile, int32_t n_knots,
                     float r_lo, float inv_step, int32_t multiply, void* stream) {
  if (dist == nullptr || in == nullptr || out == nullptr || profile == nullptr)
    return fail(INR_ERR_INVALID, "inr_radial_scale: null argument");
  if (int rc = scale_rows_count_check(n, "inr_radial_scale")) return rc;
  if (n_knots < 2 || n_knots > INR_RADIAL_KNOTS_MAX)
    return fail(INR_ERR_INVALID, "inr_radial_scale: n_knots = %d (2..%d)", (int)n_knots, INR_RADIAL_KNOTS_MAX);
  if (!std::isfinite(r_lo)) return fail(INR_ERR_INVALID, "inr_radial_scale: r_lo = %g (must be finite)", (double)r_lo);
  if (!std::isfinite(inv_step) || !(inv_step > 0.f))
    return fail(INR_ERR_INVALID, "inr_radial_scale: inv_step = %g (must be finite and positive)", (double)inv_step);
  if (((uintptr_t)profile & 3u) != 0) return fail(INR_ERR_INVALID, "inr_radial_scale: profile must be 4-byte aligned");
  if (int rc = scale_rows_layout_check(dist, in, out, n, "inr_radial_scale")) return rc;
  if (ranges_overlap(out, n * 8, profile, (int64_t)n_knots * 4))
    return fail(INR_ERR_INVALID, "inr_radial_scale: out overlaps profile");
  hipError_t e = inr::launch_radial_scale(dist, in, out, n, profile, n_knots, r_lo, inv_step, multiply != 0,
                                          (hipStream_t)stream);
  return hip_done(e, "inr_radial_scale");
}

// ---- learned radial gain (inr_gain.hip) ----
int inr_gain_loss_grad(const inr_loss_desc* loss, const float* y, const float* s, const float* gt, const uint8_t* mask,
                       int64_t B, float* res, float* loss_out, float* dy, float* ds, void* stream) {
  if (loss == nullptr || y == nullptr || s == nullptr || gt == nullptr || loss_out == nullptr || dy == nullptr ||
      ds == nullptr)
    return fail(INR_ERR_INVALID, "inr_gain_loss_grad: null argument");
  if (loss->kind < INR_LOSS_L2_HALF || loss->kind > INR_LOSS_CENTER)
    return fail(INR_ERR_INVALID, "inr_gain_loss_grad: loss kind %d", loss->kind);
  if (B <= 0) return fail(INR_ERR_INVALID, "inr_gain_loss_grad: B = %lld", (long long)B);
  if ((((uintptr_t)y | (uintptr_t)gt | (uintptr_t)dy | (uintptr_t)res) & 7u) != 0 || (((uintptr_t)s | (uintptr_t)ds) & 3u) != 0)
    return fail(INR_ERR_INVALID, "inr_gain_loss_grad: y / gt / dy / res must be 8-byte aligned ([B,2] rows move as one "
                "load), s / ds 4-byte aligned");
  LossDesc ld;
  to_loss_desc(loss, &ld);
  hipError_t e = inr::launch_gain_loss_grad(ld, y, s, gt, mask, B, res, loss_out, dy, ds, (hipStream_t)stream);
  return hip_done(e, "inr_gain_loss_grad");
}

int inr_gain_apply(const float* y, const float* s, int64_t B, float* res, void* stream) {
  if (y == nullptr || s == nullptr || res == nullptr) return fail(INR_ERR_INVALID, "inr_gain_apply: null argument");
  if (B <= 0) return fail(INR_ERR_INVALID, "inr_gain_apply: B = %lld", (long long)B);
  if ((((uintptr_t)y | (uintptr_t)res) & 7u) != 0 || ((uintptr_t)s & 3u) != 0)
    return fail(INR_ERR_INVALID, "inr_gain_apply: y / res must be 8-byte aligned, s 4-byte aligned");
  hipError_t e = inr::launch_gain_apply(y, s, B, res, (hipStream_t)stream);
  return hip_done(e, "inr_gain_apply");
}

// ---- mixture of heads (inr_mix.hip) ----
static_assert(INR_MIX_MAX_HEADS == inr::MIX_MAX_HEADS && INR_MIX_BLOCKS == inr::MIX_BLOCKS &&
                  INR_MIX_PARTIALS == inr::MIX_PARTIALS &&
                  INR_MIX_PARTIALS + (INR_MIX_MAX_HEADS + 1) * INR_MIX_BLOCKS <= INR_LOSS_WORDS,
              "inr_abi.h and inr_aux.h disagree");

// the descriptor's own fields (n_heads, the y table, and with `grad` the radii, inv_count and the dy table) -> a
static int mix_desc_check(const inr_mix_desc* mix, bool grad, inr::MixArgs* a, const char* who) {
  const int K = mix->n_heads;
  if (K < 2 || K > INR_MIX_MAX_HEADS) return fail(INR_ERR_INVALID, "%s: n_heads = %d (2..%d)", who, K, INR_MIX_MAX_HEADS);
  memset(a, 0, sizeof(*a));
  a->n_heads = K;
  a->detach = mix->detach != 0;
  a->clamp = mix->clamp != 0;
  for (int k = 0; k < K; ++k) {
    if (mix->y[k] == nullptr || (grad && mix->dy[k] == nullptr)) return fail(INR_ERR_INVALID, "%s: null table entry %d", who, k);
    if (((uintptr_t)mix->y[k] & 7u) != 0 || (grad && ((uintptr_t)mix->dy[k] & 7u) != 0))
      return fail(INR_ERR_INVALID, "%s: y[%d] / dy[%d] must be 8-byte aligned ([B,2] rows move as one load)", who, k, k);
    a->y[k] = mix->y[k];
    a->dy[k] = grad ? mix->dy[k] : nullptr;
  }
  if (!grad) return INR_OK;
  for (int k = 0; k <= K; ++k) {
    if (!(mix->radii[k] == mix->radii[k])) return fail(INR_ERR_INVALID, "%s: radii[%d] is NaN", who, k);
    if (k > 0 && !(mix->radii[k] > mix->radii[k - 1]))
      return fail(INR_ERR_INVALID, "%s: radii[%d] = %g is not above radii[%d] = %g (radii must increase)", who, k,
                  (double)mix->radii[k], k - 1, (double)mix->radii[k - 1]);
    if (!std::isfinite(mix->inv_count[k]) || mix->inv_count[k] < 0.f)
      return fail(INR_ERR_INVALID, "%s: inv_count[%d] = %g (must be finite and not negative)", who, k,
                  (double)mix->inv_count[k]);
    a->radii[k] = mix->radii[k];
    a->inv_count[k] = mix->inv_count[k];
  }
  return INR_OK;
}

int inr_mix_loss_grad(const inr_loss_desc* loss, const inr_mix_desc* mix, const float* w, const float* gt,
                      const float* dist, const uint8_t* mask, int64_t B, float* res, float* loss_out, float* dw,
                      void* stream) {
  if (loss == nullptr || mix == nullptr || w == nullptr || gt == nullptr || dist == nullptr || loss_out == nullptr ||
      dw == nullptr)
    return fail(INR_ERR_INVALID, "inr_mix_loss_grad: null argument");
  if (loss->kind < INR_LOSS_L2_HALF || loss->kind > INR_LOSS_CENTER)
    return fail(INR_ERR_INVALID, "inr_mix_loss_grad: loss kind %d", loss->kind);
  if (B <= 0) return fail(INR_ERR_INVALID, "inr_mix_loss_grad: B = %lld", (long long)B);
  inr::MixArgs a;
  if (int rc = mix_desc_check(mix, true, &a, "inr_mix_loss_grad")) return rc;
  if ((((uintptr_t)gt | (uintptr_t)res) & 7u) != 0 || (((uintptr_t)w | (uintptr_t)dw | (uintptr_t)dist) & 3u) != 0)
    return fail(INR_ERR_INVALID, "inr_mix_loss_grad: gt / res must be 8-byte aligned ([B,2] rows move as one load), "
                "w / dw / dist 4-byte aligned");
  LossDesc ld;
  to_loss_desc(loss, &ld);
  hipError_t e = inr::launch_mix_loss_grad(ld, a, w, gt, dist, mask, B, res, loss_out, dw, (hipStream_t)stream);
  return hip_done(e, "inr_mix_loss_grad");
}

int inr_mix_apply(const inr_mix_desc* mix, const float* w, int64_t B, float* res, void* stream) {
  if (mix == nullptr || w == nullptr || res == nullptr) return fail(INR_ERR_INVALID, "inr_mix_apply: null argument");
  if (B <= 0) return fail(INR_ERR_INVALID, "inr_mix_apply: B = %lld", (long long)B);
  inr::MixArgs a;
  if (int rc = mix_desc_check(mix, false, &a, "inr_mix_apply")) return rc;
  if (((uintptr_t)res & 7u) != 0 || ((uintptr_t)w & 3u) != 0)
    return fail(INR_ERR_INVALID, "inr_mix_apply: res must be 8-byte aligned, w 4-byte aligned");
  hipError_t e = inr::launch_mix_apply(a, w, B, res, (hipStream_t)stream);
  return hip_done(e, "inr_mix_apply");
}

// ---- SENSE-model fits (inr_sense.hip) ----
// what the two entries share: the extents, the shift switch and the factor; *plane_bytes = H * W * 8
static int sense_dims_check(int32_t G, int64_t H, int64_t W, float scale, int32_t shift, int64_t* plane_bytes,
                            const char* who) {
  if (G < 1 || H < 1 || W < 1 || H > (1LL << 30) || W > (1LL << 30) || H * W > (1LL << 40) / G)
    return fail(INR_ERR_INVALID, "%s: G %d, H %lld, W %lld (each >= 1, G * H * W <= 2^40)", who, (int)G, (long long)H,
                (long long)W);
  if (shift != 0 && shift != 1) return fail(INR_ERR_INVALID, "%s: shift = %d (0 or 1)", who, (int)shift);
  if (!std::isfinite(scale)) return fail(INR_ERR_INVALID, "%s: scale = %g (must be finite)", who, (double)scale);
  *plane_bytes = H * W * 8;
  return INR_OK;
}

int inr_sense_apply(const float* img, const float* sens, int32_t G, int64_t H, int64_t W, float scale, int32_t shift,
                    float* x, void* stream) {
  if (img == nullptr || sens == nullptr || x == nullptr) return fail(INR_ERR_INVALID, "inr_sense_apply: null argument");
  int64_t pb;
  if (int rc = sense_dims_check(G, H, W, scale, shift, &pb, "inr_sense_apply")) return rc;
  if ((((uintptr_t)img | (uintptr_t)sens | (uintptr_t)x) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_sense_apply: img / sens / x must be 8-byte aligned ((re, im) pairs move as one load)");
  if (ranges_overlap(x, G * pb, img, pb) || ranges_overlap(x, G * pb, sens, G * pb))
    return fail(INR_ERR_INVALID, "inr_sense_apply: x overlaps img or sens (a shifted write has no in-place form)");
  hipError_t e = inr::launch_sense_apply(img, sens, G, H, W, scale, shift, x, (hipStream_t)stream);
  return hip_done(e, "inr_sense_apply");
}

int inr_sense_grad(const float* img, const float* sens, const float* gx, int32_t G, int64_t H, int64_t W, float scale,
                   int32_t shift, float* dimg, float* dsens, void* stream) {
  if (img == nullptr || sens == nullptr || gx == nullptr || dimg == nullptr || dsens == nullptr)
    return fail(INR_ERR_INVALID, "inr_sense_grad: null argument");
  int64_t pb;
  if (int rc = sense_dims_check(G, H, W, scale, shift, &pb, "inr_sense_grad")) return rc;
  if ((((uintptr_t)img | (uintptr_t)sens | (uintptr_t)gx | (uintptr_t)dimg | (uintptr_t)dsens) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_sense_grad: img / sens / gx / dimg / dsens must be 8-byte aligned ((re, im) pairs "
                "move as one load)");
  if (ranges_overlap(dimg, pb, img, pb) || ranges_overlap(dimg, pb, sens, G * pb) || ranges_overlap(dimg, pb, gx, G * pb) ||
      ranges_overlap(dsens, G * pb, img, pb) || ranges_overlap(dsens, G * pb, sens, G * pb) ||
      ranges_overlap(dsens, G * pb, gx, G * pb) || ranges_overlap(dimg, pb, dsens, G * pb))
    return fail(INR_ERR_INVALID, "inr_sense_grad: dimg / dsens overlaps another buffer");
  hipError_t e = inr::launch_sense_grad(img, sens, gx, G, H, W, scale, shift, dimg, dsens, (hipStream_t)stream);
  return hip_done(e, "inr_sense_grad");
}

// ---- SENSE fits on calibrated coil maps (inr_sense_calib.hip) ----
static_assert(INR_SENSE_CALIB_MAX == inr::SENSE_CALIB_MAX, "inr_abi.h and inr_aux.h disagree");

int inr_sense_lowres(const float* kc, const float* ey, const float* ex, int32_t C, int32_t a, int32_t b, int64_t Ho,
                     int64_t Wo, float* out, void* stream) {
  if (kc == nullptr || ey == nullptr || ex == nullptr || out == nullptr)
    return fail(INR_ERR_INVALID, "inr_sense_lowres: null argument");
  if (a < 2 || a > INR_SENSE_CALIB_MAX || b < 2 || b > INR_SENSE_CALIB_MAX)
    return fail(INR_ERR_INVALID, "inr_sense_lowres: a = %d, b = %d (each 2..%d)", (int)a, (int)b, INR_SENSE_CALIB_MAX);
  if (C < 1 || C > 65535 || Ho < 1 || Wo < 1 || Ho > (1LL << 20) || Wo > (1LL << 20) || Ho * Wo > (1LL << 40) / C)
    return fail(INR_ERR_INVALID, "inr_sense_lowres: C %d, Ho %lld, Wo %lld (C in 1..65535, Ho and Wo in 1..2^20, "
                "C * Ho * Wo <= 2^40)", (int)C, (long long)Ho, (long long)Wo);
  if ((((uintptr_t)kc | (uintptr_t)ey | (uintptr_t)ex | (uintptr_t)out) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_sense_lowres: kc / ey / ex / out must be 8-byte aligned ((re, im) pairs move as one "
                "load)");
  const int64_t out_bytes = (int64_t)C * Ho * Wo * 8;
  if (ranges_overlap(out, out_bytes, kc, (int64_t)C * a * b * 8) || ranges_overlap(out, out_bytes, ey, a * Ho * 8) ||
      ranges_overlap(out, out_bytes, ex, b * Wo * 8))
    return fail(INR_ERR_INVALID, "inr_sense_lowres: out overlaps kc, ey or ex");
  hipError_t e = inr::launch_sense_lowres(kc, ey, ex, C, a, b, Ho, Wo, out, (hipStream_t)stream);
  return hip_done(e, "inr_sense_lowres");
}

int inr_sense_maps(const float* low, int32_t C, int64_t P, float floor, float* maps, float* rss, void* stream) {
  if (low == nullptr || maps == nullptr || rss == nullptr) return fail(INR_ERR_INVALID, "inr_sense_maps: null argument");
  if (C < 1 || P < 1 || P > (1LL << 40) / C)
    return fail(INR_ERR_INVALID, "inr_sense_maps: C %d, P %lld (each >= 1, C * P <= 2^40)", (int)C, (long long)P);
  if (!(floor >= 0.f && floor < 1.f))
    return fail(INR_ERR_INVALID, "inr_sense_maps: floor = %g (0 <= floor < 1)", (double)floor);
  if ((((uintptr_t)low | (uintptr_t)maps) & 7u) != 0 || ((uintptr_t)rss & 3u) != 0)
    return fail(INR_ERR_INVALID, "inr_sense_maps: low / maps must be 8-byte aligned ((re, im) pairs move as one load), rss "
                "4-byte aligned");
  const int64_t cb = (int64_t)C * P * 8;
  if (ranges_overlap(maps, cb, low, cb) || ranges_overlap(rss, P * 4, low, cb) || ranges_overlap(rss, P * 4, maps, cb))
    return fail(INR_ERR_INVALID, "inr_sense_maps: maps / rss overlaps another buffer");
  hipError_t e = inr::launch_sense_maps(low, C, P, floor, maps, rss, (hipStream_t)stream);
  return hip_done(e, "inr_sense_maps");
}

int inr_sense_adjoint(const float* sens, const float* gx, int32_t G, int64_t H, int64_t W, float scale, int32_t shift,
                      float* dimg, void* stream) {
  if (sens == nullptr || gx == nullptr || dimg == nullptr) return fail(INR_ERR_INVALID, "inr_sense_adjoint: null argument");
  int64_t pb;
  if (int rc = sense_dims_check(G, H, W, scale, shift, &pb, "inr_sense_adjoint")) return rc;
  if ((((uintptr_t)sens | (uintptr_t)gx | (uintptr_t)dimg) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_sense_adjoint: sens / gx / dimg must be 8-byte aligned ((re, im) pairs move as one "
                "load)");
  if (ranges_overlap(dimg, pb, sens, G * pb) || ranges_overlap(dimg, pb, gx, G * pb))
    return fail(INR_ERR_INVALID, "inr_sense_adjoint: dimg overlaps sens or gx");
  hipError_t e = inr::launch_sense_adjoint(sens, gx, G, H, W, scale, shift, dimg, (hipStream_t)stream);
  return hip_done(e, "inr_sense_adjoint");
}

// ---- total-variation prior on the image of a SENSE fit (inr_image_tv.hip) ----
static_assert(INR_IMAGE_TV_BLOCKS == inr::IMAGE_TV_BLOCKS && INR_IMAGE_TV_PARTIALS == inr::IMAGE_TV_PARTIALS &&
                  INR_IMAGE_TV_PARTIALS % 2 == 0 && INR_IMAGE_TV_PARTIALS + 2 * INR_IMAGE_TV_BLOCKS <= INR_LOSS_WORDS,
              "inr_abi.h and inr_aux.h disagree, or the fp64 partials leave the INR_LOSS_WORDS words");

int inr_image_tv_grad(const float* img, int64_t H, int64_t W, float weight, float eps, int32_t accumulate, float* loss_out,
                      float* dimg, void* stream) {
  if (img == nullptr || loss_out == nullptr) return fail(INR_ERR_INVALID, "inr_image_tv_grad: null argument");
  if (H < 1 || W < 1 || H > (1LL << 30) || W > (1LL << 30) || H * W > (1LL << 40))
    return fail(INR_ERR_INVALID, "inr_image_tv_grad: H %lld, W %lld (each >= 1, H * W <= 2^40)", (long long)H, (long long)W);
  if (!std::isfinite(eps) || eps < 0.f) return fail(INR_ERR_INVALID, "inr_image_tv_grad: eps = %g (finite and >= 0)", (double)eps);
  if (!std::isfinite(weight)) return fail(INR_ERR_INVALID, "inr_image_tv_grad: weight = %g (must be finite)", (double)weight);
  if (accumulate != 0 && accumulate != 1)
    return fail(INR_ERR_INVALID, "inr_image_tv_grad: accumulate = %d (0 or 1)", (int)accumulate);
  if ((((uintptr_t)img | (uintptr_t)dimg | (uintptr_t)loss_out) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_image_tv_grad: img / dimg / loss_out must be 8-byte aligned ((re, im) pairs move as "
                "one load; loss_out holds fp64 partials)");
  const int64_t pb = H * W * 8, lb = (int64_t)INR_LOSS_WORDS * 4;
  if (ranges_overlap(loss_out, lb, img, pb) ||
      (dimg != nullptr && (ranges_overlap(dimg, pb, img, pb) || ranges_overlap(dimg, pb, loss_out, lb))))
    return fail(INR_ERR_INVALID, "inr_image_tv_grad: dimg / loss_out overlaps another buffer");
  hipError_t e = inr::launch_image_tv_grad(img, H, W, weight, eps, accumulate != 0, loss_out, dimg, (hipStream_t)stream);
  return hip_done(e, "inr_image_tv_grad");
}

// ---- focal frequency loss (inr_loss_focal.hip) ----
static_assert(INR_FOCAL_BLOCKS == inr::FOCAL_BLOCKS && INR_FOCAL_PARTIALS == inr::FOCAL_PARTIALS &&
                  INR_FOCAL_MAXIMA == inr::FOCAL_MAXIMA && INR_FOCAL_NMAX == inr::FOCAL_NMAX &&
                  INR_FOCAL_NMAX < INR_LOSS_WORDS, "inr_abi.h and inr_aux.h disagree");

int inr_focal_loss_grad(const inr_focal_desc* d, const float* out, const float* gt, const uint8_t* mask, int64_t B,
                        float* loss_out, float* dout, void* stream) {
  if (d == nullptr || out == nullptr || gt == nullptr || loss_out == nullptr)
    return fail(INR_ERR_INVALID, "inr_focal_loss_grad: null argument");
  if (B <= 0) return fail(INR_ERR_INVALID, "inr_focal_loss_grad: B = %lld", (long long)B);
  if (!std::isfinite(d->alpha) || !(d->alpha > 0.f))
    return fail(INR_ERR_INVALID, "inr_focal_loss_grad: alpha = %g (must be finite and > 0)", (double)d->alpha);
  if (!std::isfinite(d->loss_weight) || !std::isfinite(d->inv_count))
    return fail(INR_ERR_INVALID, "inr_focal_loss_grad: loss_weight = %g, inv_count = %g (must be finite)",
                (double)d->loss_weight, (double)d->inv_count);
  if ((((uintptr_t)out | (uintptr_t)gt | (uintptr_t)dout) & 7u) != 0)
    return fail(INR_ERR_INVALID, "inr_focal_loss_grad: out / gt / dout must be 8-byte aligned ([B,2] rows move as one load)");
  inr::FocalArgs a;
  a.alpha = d->alpha;
  a.log_matrix = d->log_matrix != 0;
  a.loss_weight = d->loss_weight;
  a.inv_count = d->inv_count;
  hipError_t e = inr::launch_focal_loss_grad(a, out, gt, mask, B, loss_out, dout, (hipStream_t)stream);
  return hip_done(e, "inr_focal_loss_grad");
}

// ---- coil compression (inr_coils.hip) ----
static_assert(INR_COIL_MAX == inr::COIL_MAX && INR_COIL_TILE_PIXELS == inr::COIL_TILE_PIXELS,
              "inr_abi.h and inr_aux.h disagree");

static int coil_pixels_check(int64_t N, const char* who) {
  if (N < 1 || N >= (1LL << 31)) return fail(INR_ERR_INVALID, "%s: N = %lld (1 <= N < 2^31 pixels per call)", who, (long long)N);
  return INR_OK;
}

int inr_coil_gram_scratch(int32_t C, int64_t N, int64_t* scratch_doubles) {
  if (scratch_doubles == nullptr) return fail(INR_ERR_INVALID, "inr_coil_gram_scratch: null argument");
  if (int rc = coil_count_check(C, "C", "inr_coil_gram_scratch")) return rc;
  if (int rc = coil_pixels_check(N, "inr_coil_gram_scratch")) return rc;
  *scratch_doubles = inr::coil_gram_scratch_doubles(C, N);
  return INR_OK;
}

int inr_coil_gram(const float* data, int32_t C, int64_t N, double* gram, double* scratch, int64_t scratch_doubles,
                  void* stream) {
  if (data == nullptr || gram == nullptr || scratch == nullptr) return fail(INR_ERR_INVALID, "inr_coil_gram: null argument");
  if (int rc = coil_count_check(C, "C", "inr_coil_gram")) return rc;
  if (int rc = coil_pixels_check(N, "inr_coil_gram")) return rc;
  if (((uintptr_t)data & 7u) != 0) return fail(INR_ERR_INVALID, "inr_coil_gram: data is not 8-byte aligned");
  const int64_t need = inr::coil_gram_scratch_doubles(C, N);
  if (scratch_doubles < need)
    return fail(INR_ERR_INVALID, "inr_coil_gram: scratch holds %lld doubles, C = %d, N = %lld need %lld",
                (long long)scratch_doubles, (int)C, (long long)N, (long long)need);
  hipError_t e = inr::launch_coil_gram(data, C, N, gram, scratch, (hipStream_t)stream);
  return hip_done(e, "inr_coil_gram");
}

int inr_coil_apply(const float* in, const float* A, int32_t M, int32_t K, int64_t N, float* out, void* stream) {
  if (in == nullptr || A == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_coil_apply: null argument");
  if (int rc = coil_count_check(M, "M", "inr_coil_apply")) return rc;
  if (int rc = coil_count_check(K, "K", "inr_coil_apply")) return rc;
  if (int rc = coil_pixels_check(N, "inr_coil_apply")) return rc;
  if ((((uintptr_t)in | (uintptr_t)out) & 7u) != 0) return fail(INR_ERR_INVALID, "inr_coil_apply: in / out is not 8-byte aligned");
  const int64_t in_bytes = (int64_t)K * N * 8, out_bytes = (int64_t)M * N * 8, a_bytes = (int64_t)M * K * 8;
  if (ranges_overlap(out, out_bytes, in, in_bytes))
    return fail(INR_ERR_INVALID, "inr_coil_apply: out overlaps in (every output row reads every input row: no in-place form)");
  if (ranges_overlap(out, out_bytes, A, a_bytes)) return fail(INR_ERR_INVALID, "inr_coil_apply: out overlaps A");
  hipError_t e = inr::launch_coil_apply(in, A, M, K, N, out, (hipStream_t)stream);
  return hip_done(e, "inr_coil_apply");
}

int inr_adam_schedule(double lr, double beta1, double beta2, int32_t n, float* host_out) {
  if (host_out == nullptr || n < 1) return fail(INR_ERR_INVALID, "inr_adam_schedule: null table or n < 1");
  for (int32_t t = 0; t < n; ++t) adam_bias_terms(lr, beta1, beta2, t + 1, host_out + 2 * t, host_out + 2 * t + 1);
  return INR_OK;
}

int inr_adam_step_dev(const inr_plan* plan, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                      float* packed, const float* sched, int32_t n_sched, int32_t* step_dev, double beta1,
                      double beta2, double eps, double weight_decay, double l1, double l2, void* stream) {
  if (plan == nullptr || params == nullptr || grads == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr ||
      packed == nullptr || sched == nullptr || step_dev == nullptr)
    return fail(INR_ERR_INVALID, "inr_adam_step_dev: null argument");
  if (n_sched < 1) return fail(INR_ERR_INVALID, "inr_adam_step_dev: empty schedule");
  if (int rc = check_real_penalty(plan, l1, l2, "inr_adam_step_dev")) return rc;
  inr::AdamArgs aa = adam_args(beta1, beta2, eps, weight_decay, l1, l2);
  aa.sched = sched;
  aa.step_dev = step_dev;
  aa.n_sched = n_sched;
  hipError_t e = inr::launch_adam_pack(plan->nd, params, grads, exp_avg, exp_avg_sq, packed, aa, (hipStream_t)stream);
  if (e == hipSuccess) e = inr::launch_step_advance(step_dev, (hipStream_t)stream);
  if (e == hipSuccess) images_note(plan, IMG_EV_PACK, inr::IMG_ALL, (hipStream_t)stream);
  return hip_done(e, "inr_adam_step_dev");
}

int inr_adam_step(const inr_plan* plan, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                  float* packed, double lr, double beta1, double beta2, double eps, double weight_decay,
                  double l1, double l2, int32_t step, void* stream) {
  if (plan == nullptr || params == nullptr || grads == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr ||
      packed == nullptr)
    return fail(INR_ERR_INVALID, "inr_adam_step: null argument");
  if (step < 1) return fail(INR_ERR_INVALID, "inr_adam_step: step %d (counts from 1)", step);
  if (int rc = check_real_penalty(plan, l1, l2, "inr_adam_step")) return rc;
  inr::AdamArgs aa = adam_args(beta1, beta2, eps, weight_decay, l1, l2);
  adam_bias_terms(lr, beta1, beta2, step, &aa.step_size, &aa.bc2_sqrt);
  hipError_t e = inr::launch_adam_pack(plan->nd, params, grads, exp_avg, exp_avg_sq, packed, aa, (hipStream_t)stream);
  if (e == hipSuccess) images_note(plan, IMG_EV_PACK, inr::IMG_ALL, (hipStream_t)stream);
  return hip_done(e, "inr_adam_step");
}

int inr_reg_grad(const inr_plan* plan, const float* params, float* grads, int64_t lo, int64_t hi, double l1, double l2,
                 const float* l2_dir, void* stream) {
  if (plan == nullptr || params == nullptr || grads == nullptr) return fail(INR_ERR_INVALID, "inr_reg_grad: null argument");
  if (lo < 0 || hi < lo || hi > plan->nd.P)
    return fail(INR_ERR_INVALID, "inr_reg_grad: entries [%lld, %lld) of %d", (long long)lo, (long long)hi, plan->nd.P);
  if (l2 != 0.0 && l2_dir == nullptr && has_complex_tensors(plan->nd))
    return fail(INR_ERR_INVALID, "inr_reg_grad: l2 on a plan with complex64 tensors needs l2_dir (conj(S) / |S|)");
  hipError_t e = inr::launch_reg_grad(plan->nd, params, grads, (int)lo, (int)hi, (float)l1, (float)l2, l2_dir,
                                      (hipStream_t)stream);
  return hip_done(e, "inr_reg_grad");
}

int inr_adam_step_shard(const inr_plan* plan, float* params, const float* grads_shard, float* exp_avg,
                        float* exp_avg_sq, int64_t lo, int64_t hi, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double l1, double l2, int32_t step, void* stream) {
  if (plan == nullptr || params == nullptr || grads_shard == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr)
    return fail(INR_ERR_INVALID, "inr_adam_step_shard: null argument");
  if (step < 1) return fail(INR_ERR_INVALID, "inr_adam_step_shard: step %d (counts from 1)", step);
  if (int rc = check_real_penalty(plan, l1, l2, "inr_adam_step_shard")) return rc;
  if (lo < 0 || hi < lo || hi > plan->nd.P)
    return fail(INR_ERR_INVALID, "inr_adam_step_shard: entries [%lld, %lld) of %d", (long long)lo, (long long)hi,
                plan->nd.P);
  inr::AdamArgs aa = adam_args(beta1, beta2, eps, weight_decay, l1, l2);
  adam_bias_terms(lr, beta1, beta2, step, &aa.step_size, &aa.bc2_sqrt);
  hipError_t e = inr::launch_adam_shard(plan->nd, params, grads_shard, exp_avg, exp_avg_sq, (int)lo, (int)hi, aa,
                                        (hipStream_t)stream);
  return hip_done(e, "inr_adam_step_shard");
}

}  // extern "C"
