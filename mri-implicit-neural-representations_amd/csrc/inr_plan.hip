// inr_plan.hip -- plan creation of the C-ABI (include/inr_abi.h): layer geometry, the flat, slab and packed-image offsets,
// the weight-gradient route, the gradient-scale state of bf16 plans; and the calling thread's error text.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "inr_host.h"
#include "inr_stash.h"
#include "inr_w2.h"

namespace {

thread_local char g_err[512] = "";

// the stash family (inr_stash.h) of a plain MLP's hidden activation
inline inr::StashFamily stash_family(int hact) {
  return hact == ACT_GABOR2D ? inr::STASH_GABOR2D : (hact == ACT_GABOR ? inr::STASH_GABOR : inr::STASH_REAL);
}

// smallest built block count that holds `need` 32-row blocks (narrower nets run zero-padded), or -1
inline int pick_nb(int need, std::initializer_list<int> built) {
  for (int nb : built)
    if (nb >= need) return nb;
  return -1;
}

}  // namespace

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(INR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// gradient-scale state of a bf16 plan on the current device (inr_w2.h): S = mult = S_used = 1, amax = 0 for both kinds of
// step.  Allocated with the plan; moved if the plan is later driven on another device.
float* dz_state_alloc(const inr_plan* p) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  if (p->dz_state != nullptr && p->dz_dev == dev) return p->dz_state;
  if (p->dz_state != nullptr) (void)hipFree(p->dz_state);
  p->dz_state = nullptr;
  p->dz_ready[0] = p->dz_ready[1] = false;
  const float init[W2_STATE_FLOATS] = {1.f, 0.f, 1.f, 1.f, 1.f, 0.f, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (hipMalloc(reinterpret_cast<void**>(&p->dz_state), sizeof(init)) != hipSuccess) {
    p->dz_state = nullptr;
    return nullptr;
  }
  if (hipMemcpy(p->dz_state, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p->dz_state);
    p->dz_state = nullptr;
    return nullptr;
  }
  p->dz_dev = dev;
  return p->dz_state;
}

// Does this call have to find its gradient scale first (a pass of the kernel whose stash nobody reads, then the roll)?
// Yes for a plan's first step of a kind, and when what the remembered scale was derived from no longer applies: another
// loss (fused steps normalise the batch size away, not the loss), or -- split steps, whose d(loss)/d(out) carries the
// 1 / count -- a batch more than twice or less than half as large.  From then on the scale follows the gradient from step
// to step (dz_state_roll) with 2^10.8 of headroom above the window it aims for (inr_w2.h W2_DZ_TARGET_EXP) -- a calibration
// pass is not counted as a clipped / flushed step (its roll gets no counters).
bool dz_needs_calibration(const inr_plan* p, int kind, int64_t rows, int loss_kind) {
  return !p->dz_ready[kind] || (kind == 0 ? p->dz_loss[0] != loss_kind
                                          : (rows > 2 * p->dz_rows[1] || 2 * rows < p->dz_rows[1]));
}
// ... remembered once the kernels that use (or found) the scale have been launched
void dz_mark(const inr_plan* p, int kind, int64_t rows, int loss_kind) {
  p->dz_ready[kind] = true;
  p->dz_rows[kind] = rows;
  p->dz_loss[kind] = loss_kind;
}
// ---- the plan's weight-image state (inr_host.h) ----
bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

int image_sets_skip(const inr_plan* plan, int reads, hipStream_t st) {
  if (!plan->nd.rs) return 0;
  if (stream_capturing(st)) {
    plan->img_eager = true;
    return 0;
  }
  return plan->img_eager || !lazy_pack_enabled() ? 0 : (inr::IMG_ALL & ~reads);
}

void images_note(const inr_plan* plan, int event, int sets, hipStream_t st) {
  if (!plan->nd.rs) return;
  if (stream_capturing(st)) {  // nothing ran: the launch lives in a graph, which writes (or re-packs) on every replay
    plan->img_eager = true;
    return;
  }
  plan->img_valid = image_sets_after(plan->img_valid, event, sets);
}

// items and the flat-gradient range [lo, hi) of the layers the batch-level dW GEMM covers -- everything of its arguments
// that no batch changes; false: the plan keeps its in-kernel dW passes
static bool dw_gemm_items(const NetDesc& nd, inr::DwGemmArgs* g, inr::SlabSplit* split) {
  memset(g, 0, sizeof(*g));
  split->lo = split->hi = split->n2 = 0;
  split->mask = 0;
  const bool g2d = nd.hact == ACT_GABOR2D;
  if (nd.bf16) return false;
  if (nd.mfn_n != 0) {
    // 512-wide filter networks (inr_mfn_wide_impl.h):  F_t: g_u_t (stash slot LCOS of stage t) x encoder features,
    // t < S;  L_{i-1}: g_l_i (slot F of stage i) x h_{i-1} (slot HH of stage i-1), 1 <= i < S.  Their flat ranges
    // interleave with heads and Gabor centres, so the reduction learns the covered layers as a bit mask.
    if (nd.NB != 16) return false;
    const int S = nd.mfn_stages, n = nd.mfn_n;
    const inr::MfnStash st(nd.NB, 32 * nd.NW);
    if (2 * S - 1 > INR_DWG_MAX_ITEMS) return false;
    g->TL = 64, g->WB = 4;
    g->save_floats_per_tile = nd.save_floats_per_tile, g->slab_floats = nd.slab_floats;
    int k = 0;
    unsigned mask = 0;
    for (int t = 0; t < 2 * S - 1; ++t) {
      const int i = t - S + 1, l = t < S ? t : n + 1 + (i - 1);
      const LayerDesc& L = nd.L[l];
      inr::DwGemmItem& it = g->it[k++];
      it.g_off = (int)(t < S ? st.slot(t, st.LCOS) : st.slot(i, st.F));
      it.h_off = (int)(t < S ? st.enc(S) : st.slot(i - 1, st.HH));
      it.gw_off = L.gw_off, it.gb_off = L.gb_off, it.Mblk = 16, it.Kblk = L.Kblk, it.K = L.K;
      mask |= 1u << l;
    }
    g->n_items = k;
    split->mask = mask;
    return true;
  }
  // the plain MLP kernels, fp32: 256-row tensors (one wave per coordinate group) and the two-waves-per-group shapes
  if (!(nd.NB == 8 && !g2d) && nd.NB != 12 && nd.NB != 16) return false;
  const int TL = 32 * nd.NW, D = nd.D;
  const inr::MlpStash st(nd.NB, TL, stash_family(nd.hact));
  g->TL = TL;
  g->WB = nd.NB == 12 ? 3 : 4;
  g->save_floats_per_tile = nd.save_floats_per_tile;
  g->slab_floats = nd.slab_floats;
  int k = 0, covered = 0, lo = nd.P, hi = 0;
  auto add = [&](const LayerDesc& L, size_t g_off, size_t h_off) {
    inr::DwGemmItem& it = g->it[k++];
    it.g_off = (int)g_off, it.h_off = (int)h_off;
    it.gw_off = L.gw_off, it.gb_off = L.gb_off;
    it.Mblk = nd.NB, it.Kblk = L.Kblk, it.K = L.K;
    covered += L.wn + L.bn;
    lo = std::min(lo, std::min(L.w_off, L.b_off));
    hi = std::max(hi, std::max(L.w_off + L.wn, L.b_off + L.bn));
  };
  if (2 * D > INR_DWG_MAX_ITEMS) return false;
  if (nd.input == IN_GAUSS) add(nd.L[0], st.slot(0, st.DACT), st.enc(D));  // dZ_0 x encoder features
  for (int l = 1; l <= D - 2; ++l) {
    add(nd.L[l], st.slot(l, st.DACT), st.slot(l - 1, st.H));                        // dZ_l x h_{l-1}
    if (g2d) add(nd.L[nd.orth0 + l], st.slot(l, st.DA2), st.slot(l - 1, st.H));  // WIRE2D: dZ_orth,l x h_{l-1}
  }
  if (k == 0 || covered != hi - lo) return false;  // the covered layers must be one contiguous flat range
  g->n_items = k;
  split->lo = lo;
  split->hi = hi;
  return true;
}

// end of plan creation: where the plan's weight gradients come from (inr_plan::dw_route), and the fp32 GEMM's items
static void plan_set_dw_route(inr_plan* p) {
  p->dw_route = p->nd.bf16 ? 2 : (dw_gemm_items(p->nd, &p->gemm, &p->gemm_cover) ? 1 : 0);
}
// ---- where a plan's layers live, one rule for every family.  The builders say which layers, in which order. ----
struct Placed {
  int layer;    // index into NetDesc::L
  bool narrow;  // last / head layer: M rows.  Hidden-width layers keep all NB*32
  bool back;    // has a backward image (not the first layer, not a filter)
  bool mu;      // LT_GABOR_MU: (mu, gamma) of a Gabor filter as a (weight, bias) pair
};

// flat parameters: weight then bias of each layer, `order` = state_dict order
static void place_flat(NetDesc& nd, const int* order, int n) {
  int poff = 0;
  for (int i = 0; i < n; ++i) {
    LayerDesc& L = nd.L[order[i]];
    L.w_off = poff;
    poff += L.wn;
    L.b_off = poff;
    poff += L.bn;
  }
  nd.P = poff;
}

// gradient slab: hidden-width layers keep whole 32-row blocks (the plain dW pass stores them without a bounds test;
// padding rows receive exact zeros and are never read back); the loss sits behind the last layer
static void place_slab(NetDesc& nd, const Placed* pl, int n) {
  int goff = 0;
  for (int i = 0; i < n; ++i) {
    LayerDesc& L = nd.L[pl[i].layer];
    const int rows = pl[i].narrow ? L.M : nd.NB * 32;
    L.gw_off = goff;
    goff += rows * L.K;
    L.gb_off = goff;
    goff += pl[i].mu ? 2 * nd.NB * 32 : rows;  // LT_GABOR_MU: [s0 | T], NB*32 apart
  }
  nd.slab_loss_off = goff;
  nd.slab_floats = round_up(goff + 4, 64);
}

// packed images: forward, backward (where there is one), bias; returns their floats.  `images` false: none (-1)
static int64_t place_images(NetDesc& nd, const Placed* pl, int n, bool images) {
  int64_t pk = 0;
  for (int i = 0; i < n; ++i) {
    LayerDesc& L = nd.L[pl[i].layer];
    L.pf_off = L.pb_off = L.pbias_off = L.rf_off = L.rb_off = -1;
    if (!images) continue;
    L.pf_off = (int)pk;
    pk += (int64_t)L.Kpad8 * L.Mblk * 32;  // (Kpad8/8 groups) x Mblk x 64 lanes x 4
    if (pl[i].back) {
      L.pb_off = (int)pk;
      pk += (int64_t)L.Mpad8 * L.Kblk * 32;
    }
    L.pbias_off = (int)pk;
    pk += (pl[i].mu ? 2 : 1) * L.Mblk * 32;  // LT_GABOR_MU: [gamma | |mu_j|^2]
  }
  return pk;
}

// Multiplicative filter networks (models/mfn.py).  L[] = filters 0..n | linears 0..n-1 | heads; flat
// parameters keep the state_dict order  linear.* , output_linear(.k).* , filters.*  (SURVEY Appendix B).
static int create_mfn_plan(const inr_net_desc* d, inr_plan** out) {
  const bool multi = d->kind == INR_KIND_MSFOURIER || d->kind == INR_KIND_MSBOUNDED;
  const bool gabor = d->kind == INR_KIND_GABOR || d->kind == INR_KIND_KGABOR;
  const int n = d->depth, W = d->width;
  if (n < 1 || 2 * n + 1 + (multi ? n + 1 : 1) + (gabor ? n + 1 : 0) > INR_MAX_LAYERS)
    return fail(INR_ERR_INVALID, "inr_plan_create: MFN depth %d", n);
  const int NB = W < 1 ? -1 : pick_nb((W + 31) / 32, {1, 4, 8, 16});
  if (NB < 0)
    return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: MFN width %d (kernels are built for widths 1..512)", W);
  // The filters read their input features from a [2E'][TL] image in the stash, k-step s -> rows s (lane half 0)
  // and E' + s (half 1).  INR_INPUT_GAUSS: the fused encoder writes it, E' = enc_size.  INR_INPUT_X: the kernel
  // transposes the tile's rows of x [B,in_features] into it, E' = half of in_features rounded up to 16 (rows past
  // in_features are zero and carry zero weights).
  int Ehalf;
  if (d->input == INR_INPUT_GAUSS) {
    if (d->enc_size < 8 || (d->enc_size % 8) != 0 || d->in_features != 2 * d->enc_size)
      return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: fused gauss encoder needs in_features == 2*enc_size, "
                  "enc_size %% 8 == 0");
    Ehalf = d->enc_size;
  } else if (d->input == INR_INPUT_X) {
    if (d->in_features < 1 || d->in_features > 4096)
      return fail(INR_ERR_INVALID, "inr_plan_create: in_features %d", d->in_features);
    Ehalf = round_up(d->in_features, 16) / 2;
  } else {
    return fail(INR_ERR_INVALID, "inr_plan_create: input mode %d", d->input);
  }
  if (d->out_features < 1 || d->out_features > 4)
    return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: out_features %d outside [1,4]", d->out_features);
  inr_plan* p = new (std::nothrow) inr_plan();
  if (p == nullptr) return fail(INR_ERR_INVALID, "inr_plan_create: out of host memory");
  p->desc = *d;
  NetDesc& nd = p->nd;
  memset(&nd, 0, sizeof(nd));
  nd.NB = NB;
  nd.NW = NB == 16 ? 2 : 4;
  nd.hact = ACT_SIN;
  nd.last_act = ACT_ID;
  nd.input = d->input == INR_INPUT_GAUSS ? IN_GAUSS : IN_X;
  nd.E = Ehalf;
  nd.out_f = d->out_features;
  nd.mfn_n = n;
  if (d->kind == INR_KIND_MSBOUNDED) {
    nd.bounded = 1;  // bounds default to "everything" until inr_plan_set_bounds is called
    for (int i = 0; i < INR_MAX_LAYERS / 2; ++i) {
      nd.bound_lo[i] = -1e30f;
      nd.bound_hi[i] = 1e30f;
    }
  }
  // heads: FourierNet -> output_linear after the last stage (mfn.py:85-94); multiscale -> output_linear[i]
  // for i in output_layers = [1,3,5,7] (mfn.py:223,262-263), those beyond depth do not exist
  if (multi) {
    const int stages[4] = {1, 3, 5, 7};
    for (int k = 0; k < 4; ++k)
      if (stages[k] <= n) nd.head_stage[nd.n_heads++] = stages[k];
    if (nd.n_heads == 0) {
      delete p;
      return fail(INR_ERR_INVALID, "inr_plan_create: multiscale MFN of depth %d has no output layer", n);
    }
  } else {
    nd.n_heads = 1;
    nd.head_stage[0] = n;
  }
  nd.mfn_stages = nd.head_stage[nd.n_heads - 1] + 1;
  const int n_head_layers = multi ? n + 1 : 1;
  nd.gabor = gabor ? 1 : 0;
  nd.mu0 = (n + 1) + n + n_head_layers;
  nd.D = nd.mu0 + (gabor ? n + 1 : 0);
  nd.ND = nd.D;
  const int TL = 32 * nd.NW;
  auto fill = [&](LayerDesc& L, int K, int M, bool filter, bool head) {
    L.K = K;
    L.M = M;
    L.Kpad8 = filter ? 2 * Ehalf : NB * 32;  // == round_up(K, 8) for the gauss encoder
    L.Kblk = filter ? (K + 31) / 32 : NB;  // hidden images always span all NB blocks (zero padding)
    L.Mblk = head ? (M + 31) / 32 : NB;
    L.Mpad8 = head ? round_up(M, 8) : NB * 32;
    L.ltype = LT_REAL;
    L.wn = M * K;
    L.bn = M;
    L.korder = filter ? 1 : 0;
  };
  for (int i = 0; i <= n; ++i) {
    fill(nd.L[i], d->in_features, W, true, false);
    nd.L[i].live = i < nd.mfn_stages;
  }
  for (int i = 0; i < n; ++i) {
    fill(nd.L[n + 1 + i], W, W, false, false);
    nd.L[n + 1 + i].live = i < nd.mfn_stages - 1;
  }
  for (int i = 0; i < n_head_layers; ++i) {
    fill(nd.L[2 * n + 1 + i], W, d->out_features, false, true);
    nd.L[2 * n + 1 + i].live = 0;
  }
  for (int k = 0; k < nd.n_heads; ++k) {
    nd.head_layer[k] = 2 * n + 1 + (multi ? nd.head_stage[k] : 0);
    nd.L[nd.head_layer[k]].live = 1;
  }
  if (gabor)  // (mu_i, gamma_i) of GaborLayer i as a (weight, bias) pair: same shapes as the filter's Linear
    for (int i = 0; i <= n; ++i) {
      fill(nd.L[nd.mu0 + i], d->in_features, W, true, false);
      nd.L[nd.mu0 + i].ltype = LT_GABOR_MU;
      nd.L[nd.mu0 + i].live = 1;
    }
  // flat offsets in state_dict order: linears, heads, filters
  int order[INR_MAX_LAYERS], no = 0;
  for (int i = 0; i < n; ++i) order[no++] = n + 1 + i;
  for (int i = 0; i < n_head_layers; ++i) order[no++] = 2 * n + 1 + i;
  for (int i = 0; i <= n; ++i) {  // filters.i.mu, filters.i.gamma, filters.i.linear.weight, filters.i.linear.bias
    if (gabor) order[no++] = nd.mu0 + i;
    order[no++] = i;
  }
  place_flat(nd, order, no);
  Placed pl[INR_MAX_LAYERS];
  for (int l = 0; l < nd.D; ++l) {
    const bool filter = l <= n || l >= nd.mu0;
    pl[l] = Placed{l, /*narrow=*/l >= 2 * n + 1 && l < nd.mu0, /*back=*/!filter, /*mu=*/l >= nd.mu0};
  }
  place_slab(nd, pl, nd.D);
  p->packed_floats = place_images(nd, pl, nd.D, true);
  nd.w2_off = nd.w2_bias_off = -1;
  const inr::MfnStash st(NB, TL);
  nd.save_floats_per_tile = (int)st.floats_per_tile(nd.mfn_stages, nd.L[0].Kblk * 32);  // Kblk*32 >= 2 E'
  plan_set_dw_route(p);
  *out = p;
  return INR_OK;
}

extern "C" {

int inr_abi_version(void) { return INR_ABI_VERSION; }

int inr_last_error(char* buf, size_t cap) {
  const size_t n = strlen(g_err);
  if (buf != nullptr && cap > 0) {
    const size_t c = n < cap - 1 ? n : cap - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return (int)n;
}

int inr_plan_create(const inr_net_desc* d, inr_plan** out) {
  if (d == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_plan_create: null argument");
  *out = nullptr;
  if (d->kind == INR_KIND_FOURIER || d->kind == INR_KIND_MSFOURIER || d->kind == INR_KIND_MSBOUNDED ||
      d->kind == INR_KIND_GABOR || d->kind == INR_KIND_KGABOR)
    return create_mfn_plan(d, out);
  if (d->kind != INR_KIND_SIREN && d->kind != INR_KIND_FFN && d->kind != INR_KIND_WIRE && d->kind != INR_KIND_WIRE2D)
    return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: kind %d has no kernel yet", d->kind);
  const bool wire2d = d->kind == INR_KIND_WIRE2D;
  const bool wire = d->kind == INR_KIND_WIRE || wire2d;
  // number of Linear layers: SIREN/FFN network_depth counts all of them (networks.py:114-117);
  // WIRE's counts the hidden complex layers only, total = depth + 2 (networks.py:234-250)
  const int D = wire ? d->depth + 2 : d->depth;
  if (D < 2 || D > INR_MAX_LAYERS)
    return fail(INR_ERR_INVALID, "inr_plan_create: depth %d gives %d layers, outside [2,%d]", d->depth, D,
                INR_MAX_LAYERS);
  if (d->out_features < 1 || d->out_features > 4)
    return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: out_features %d outside [1,4]", d->out_features);
  if (d->in_features < 1) return fail(INR_ERR_INVALID, "inr_plan_create: in_features %d", d->in_features);
  if (d->width < 1) return fail(INR_ERR_INVALID, "inr_plan_create: width %d", d->width);
  // rows of the hidden activations as the kernel sees them: complex features are (Re, Im) row pairs
  const int hid = wire ? 2 * d->width : d->width;
  const int need = (hid + 31) / 32;
  const int NB = wire2d ? pick_nb(need, {2, 4, 8, 16})
                        : (wire ? pick_nb(need, {2, 4, 8, 12}) : pick_nb(need, {1, 2, 4, 8, 16}));
  int NW;
  if (wire) {
    if (NB < 0)
      return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: WIRE with %d complex hidden features (kernels are built for "
                  "up to 192 = 384 interleaved rows, network_width 256 gives 181; WIRE2D: up to 256)", d->width);
    NW = (NB == 12 || NB == 16) ? 2 : 4;  // 12 / 16 blocks: 64-coordinate tiles, two waves per coordinate group
    if (wire2d && 2 * D - 1 > INR_MAX_LAYERS)
      return fail(INR_ERR_INVALID, "inr_plan_create: WIRE2D depth %d", d->depth);
    if (d->input != INR_INPUT_X)
      return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: WIRE takes raw coordinates (input must be INR_INPUT_X)");
    if (d->last_act == INR_ACT_CTANH) {
      if (!wire2d || d->out_features > 2)
        return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: INR_ACT_CTANH is WIRE2D's last_tanh, out_features <= 2");
    } else if (d->last_act != INR_ACT_ID) {
      return fail(INR_ERR_INVALID, "inr_plan_create: WIRE's output is linear (or INR_ACT_CTANH for WIRE2D)");
    }
  } else {
    if (NB < 0)
      return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: width %d (kernels are built for widths 1..512)", d->width);
    NW = NB == 16 ? 2 : 4;
  }
  if (d->input == INR_INPUT_GAUSS) {
    if (d->enc_size < 8 || (d->enc_size % 8) != 0)
      return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: enc_size %d must be a positive multiple of 8", d->enc_size);
    if (d->in_features != 2 * d->enc_size)
      return fail(INR_ERR_INVALID, "inr_plan_create: in_features %d != 2*enc_size %d", d->in_features,
                  2 * d->enc_size);
  } else if (d->input != INR_INPUT_X) {
    return fail(INR_ERR_INVALID, "inr_plan_create: input mode %d", d->input);
  }
  if ((d->last_act < INR_ACT_ID || d->last_act > INR_ACT_SIGMOID) && !(wire2d && d->last_act == INR_ACT_CTANH))
    return fail(INR_ERR_INVALID, "inr_plan_create: last_act %d", d->last_act);
  if (d->precision != INR_PRECISION_F32 && d->precision != INR_PRECISION_BF16)
    return fail(INR_ERR_INVALID, "inr_plan_create: precision %d", d->precision);
  if (d->precision == INR_PRECISION_BF16 &&
      (d->kind != INR_KIND_SIREN || d->input != INR_INPUT_GAUSS || NB != 8 || (d->enc_size % 32) != 0 || D < 3 || D > 8 ||
       d->enc_size > 1024))
    return fail(INR_ERR_UNSUPPORTED, "inr_plan_create: the bf16 path is built for SIREN with the fused gauss encoder, "
                "hidden width 129..256, 3 to 8 layers and an encoder size that is a multiple of 32 up to 1024 (got kind %d, input "
                "%d, width %d, depth %d, enc_size %d)", d->kind, d->input, d->width, d->depth, d->enc_size);

  inr_plan* p = new (std::nothrow) inr_plan();
  if (p == nullptr) return fail(INR_ERR_INVALID, "inr_plan_create: out of host memory");
  p->desc = *d;
  NetDesc& nd = p->nd;
  memset(&nd, 0, sizeof(nd));
  nd.D = D;
  nd.NB = NB;
  nd.NW = NW;
  nd.bf16 = d->precision == INR_PRECISION_BF16 ? 1 : 0;
  nd.hact = wire2d ? ACT_GABOR2D : (wire ? ACT_GABOR : (d->kind == INR_KIND_SIREN ? ACT_SIN : ACT_RELU));
  nd.ND = wire2d ? 2 * D - 1 : D;
  nd.orth0 = D;
  nd.last_act = d->last_act;
  nd.input = d->input;
  nd.E = d->enc_size;
  nd.out_f = d->out_features;
  nd.w0 = d->w0;
  const int TL = 32 * NW;
  int order[INR_MAX_LAYERS];
  Placed pl[INR_MAX_LAYERS];
  // descriptors in flat-parameter order: WIRE2D interleaves linear / scale_orth of each layer (wire2d.py:40-47)
  for (int t = 0; t < nd.ND; ++t) {
    const int l = wire2d ? (t == nd.ND - 1 ? D - 1 : t / 2) : t;
    const bool orth = wire2d && t != nd.ND - 1 && (t & 1);
    LayerDesc& L = nd.L[orth ? nd.orth0 + l : l];
    const bool first = l == 0, last = l == D - 1;
    const bool ctanh_last = last && d->last_act == INR_ACT_CTANH;  // complex output kept: (Re, Im) row pairs
    L.K = first ? d->in_features : hid;
    L.M = last ? (ctanh_last ? 2 * d->out_features : d->out_features) : hid;
    // hidden-to-hidden products run over all NB*32 image rows (padding rows carry zero weights)
    L.Kpad8 = first ? round_up(L.K, 8) : NB * 32;
    L.Kblk = first ? (L.K + 31) / 32 : NB;  // hidden images always span all NB blocks (zero padding)
    L.Mblk = last ? (L.M + 31) / 32 : NB;
    L.Mpad8 = last ? round_up(L.M, 8) : NB * 32;
    if (!wire) {
      L.ltype = LT_REAL;
      L.wn = L.M * L.K;
      L.bn = L.M;
      L.omega = d->w0;
      L.s0 = 0.f;
    } else if (first) {
      L.ltype = LT_WIRE_FIRST;  // real weights on real coordinates (networks.py:185-188)
      L.wn = d->width * L.K;
      L.bn = d->width;
      L.omega = d->first_omega_0;
      L.s0 = d->scale_0;
    } else if (!last) {
      L.ltype = LT_WIRE_HIDDEN;
      L.wn = d->width * d->width * 2;
      L.bn = d->width * 2;
      L.omega = d->hidden_omega_0;
      L.s0 = d->scale_0;
    } else {
      // complex Linear, output.real (networks.py:247-258): only the real rows exist -- unless a complex Tanh sits
      // before .real (WIRE2D last_tanh), which needs the imaginary rows too: the hidden-layer mapping
      L.ltype = ctanh_last ? LT_WIRE_HIDDEN : LT_WIRE_LAST;
      L.wn = d->out_features * d->width * 2;
      L.bn = d->out_features * 2;
    }
    order[t] = orth ? nd.orth0 + l : l;
    pl[t] = Placed{order[t], /*narrow=*/last, /*back=*/l >= 1, /*mu=*/false};
    L.live = 1;
    L.korder = (first && d->input == INR_INPUT_GAUSS) ? 1 : 0;
  }
  place_flat(nd, order, nd.ND);
  place_slab(nd, pl, nd.ND);
  int64_t pk = place_images(nd, pl, nd.ND, !nd.bf16);  // bf16 plans keep one image set only: the panel stream (below)
  // (the encoder features and WIRE2D's gradient copy share an offset, inr_stash.h: WIRE behind the gauss encoder was
  // refused above)
  const inr::MlpStash st(NB, TL, stash_family(nd.hact));
  nd.save_floats_per_tile = (int)st.floats_per_tile(D, d->input == INR_INPUT_GAUSS ? nd.L[0].Kblk * 32 : 0);
  nd.w2_off = nd.w2_bias_off = -1;
  // Row-split fused step (inr_mlp_rs_impl.h): SIREN / FFN behind the fused gauss encoder, hidden width 129..256, encoder
  // size a multiple of 32 that leaves room in LDS.  Such plans carry a second set of fragment images (16x16x4 MFMA
  // operands); forward / backward calls keep inr_mlp_kernel and its images.
  for (int t = 0; t < INR_MAX_LAYERS; ++t) nd.L[t].rf_off = nd.L[t].rb_off = -1;
  if (!nd.bf16 && !wire && NB == 8 && d->input == INR_INPUT_GAUSS && (d->enc_size % 32) == 0 && d->enc_size <= 512) {
    nd.rs = 1;
    for (int l = 0; l <= D - 2; ++l) {
      nd.L[l].rf_off = (int)pk;
      pk += (int64_t)256 * (l == 0 ? 2 * d->enc_size : 256);
      if (l >= 1) {
        nd.L[l].rb_off = (int)pk;
        pk += (int64_t)256 * 256;
      }
    }
  }
  if (nd.bf16) {
    // the images of the bf16 plans: the "weight panels in LDS" stream (inr_w2.h) + fp32 biases; 8-bit stash
    nd.w2_off = (int)pk;  // (0: 16-byte aligned, the panels are read by 16-byte LDS-DMA pieces)
    pk += (int64_t)w2_np(D, d->enc_size) * W2_PANEL_FLOATS;
    nd.w2_bias_off = (int)pk;
    pk += (int64_t)D * 256;
    nd.save_floats_per_tile = w2_stash_dwords(D);
    // (the gradient-scale state is allocated by the first call that needs it, on that call's device: creating and sizing
    // a plan touches no GPU -- tests/test_host.py sizes bf16 workspaces on the CPU)
  }
  p->packed_floats = pk;
  p->gemm_one_class = getenv("INR_GEMM_ONE_CLASS") != nullptr;
  if (const char* e = getenv("INR_GEMM_ENC_COST")) p->gemm_enc_cost = std::max(1.0, atof(e));
  plan_set_dw_route(p);
  *out = p;
  return INR_OK;
}

int inr_plan_destroy(inr_plan* plan) {
  if (plan != nullptr && plan->side != nullptr) (void)hipStreamDestroy(plan->side);
  if (plan != nullptr && plan->fork != nullptr) (void)hipEventDestroy(plan->fork);
  if (plan != nullptr && plan->join != nullptr) (void)hipEventDestroy(plan->join);
  if (plan != nullptr && plan->dz_state != nullptr) (void)hipFree(plan->dz_state);
  delete plan;
  return INR_OK;
}

int inr_plan_sizes(const inr_plan* plan, inr_sizes* out) {
  if (plan == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_plan_sizes: null argument");
  out->n_params = plan->nd.P;
  out->packed_floats = plan->packed_floats;
  out->tile_rows = 32 * plan->nd.NW;
  out->save_bytes_per_tile = (int64_t)plan->nd.save_floats_per_tile * 4;
  out->max_blocks = kMaxBlocks;
  out->slab_floats = plan->nd.slab_floats;
  out->step_save_by_tile = plan->dw_route != 0 ? 1 : 0;
  return INR_OK;
}

int inr_plan_grad_scale_state(const inr_plan* plan, float* host_out, void* stream) {
  if (plan == nullptr || host_out == nullptr) return fail(INR_ERR_INVALID, "inr_plan_grad_scale_state: null argument");
  if (!plan->nd.bf16) return fail(INR_ERR_INVALID, "inr_plan_grad_scale_state: not an INR_PRECISION_BF16 plan");
  if (dz_state_alloc(plan) == nullptr)  // (before the first step: the initial state)
    return fail(INR_ERR_HIP, "inr_plan_grad_scale_state: no gradient-scale state on this device");
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) e = hipMemcpy(host_out, plan->dz_state, W2_STATE_FLOATS * sizeof(float), hipMemcpyDeviceToHost);
  return hip_done(e, "inr_plan_grad_scale_state");
}

int inr_plan_set_bounds(inr_plan* plan, const float* lo, const float* hi, int32_t n) {
  if (plan == nullptr || lo == nullptr || hi == nullptr) return fail(INR_ERR_INVALID, "inr_plan_set_bounds: null argument");
  if (!plan->nd.bounded) return fail(INR_ERR_INVALID, "inr_plan_set_bounds: not a MultiscaleBoundedFourier plan");
  if (n != plan->nd.mfn_n) return fail(INR_ERR_INVALID, "inr_plan_set_bounds: %d bounds for %d linears", n, plan->nd.mfn_n);
  for (int i = 0; i < n; ++i) {
    plan->nd.bound_lo[i] = lo[i];
    plan->nd.bound_hi[i] = hi[i];
  }
  return INR_OK;
}

int inr_plan_heads(const inr_plan* plan, int32_t* n_heads) {
  if (plan == nullptr || n_heads == nullptr) return fail(INR_ERR_INVALID, "inr_plan_heads: null argument");
  *n_heads = plan->nd.mfn_n > 0 ? plan->nd.n_heads : 1;
  return INR_OK;
}

}  // extern "C"
