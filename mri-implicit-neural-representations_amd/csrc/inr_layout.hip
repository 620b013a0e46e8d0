// inr_layout.hip -- the launch layout of one ABI call (CallLayout, inr_host.h): tiles and workgroups, which fused kernel
// runs and its row-split schedule, the two split-step schedules, the chunking of both weight-gradient GEMMs and the
// workspace sizes; and the ABI readers that only report it.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "inr_host.h"
#include "inr_w2.h"

// THE chunking rule: `n` tiles in equal chunks, about `target` of them
static void chunk_tiles(int64_t n, int target, int* tiles_per_chunk, int* n_chunks) {
  target = std::max(1, target);
  *tiles_per_chunk = (int)((n + target - 1) / target);
  *n_chunks = (int)((n + *tiles_per_chunk - 1) / *tiles_per_chunk);
}

// chunks of tiles [tile0, tile1) of the fp32 GEMM for about `max_wgs` workgroups (256: one per CU -- the accumulators
// then stay in registers over as many tiles as possible)
static void dw_gemm_chunk(inr::DwGemmArgs& g, int64_t tile0, int64_t tile1, int max_wgs) {
  const int64_t n = tile1 - tile0;
  g.tile0 = (int)tile0, g.n_tiles = (int)tile1;
  g.WBM = 0;
  chunk_tiles(n, max_wgs / std::max(1, inr::dw_gemm_units(g)), &g.tiles_per_chunk, &g.n_chunks);
  // short chunks (the graded 25 000 rows: K = 512 coordinates per 256 x 256 tile): half-height tiles over twice the K --
  // half as many slabs to store at the end of the launch and to reduce (inr_dw_gemm.hip)
  if (g.TL == 128 && g.WB == 4 && n > 1 && (int64_t)g.tiles_per_chunk * g.TL < 1024) {
    g.WBM = 2;
    chunk_tiles(n, max_wgs / std::max(1, inr::dw_gemm_units(g)), &g.tiles_per_chunk, &g.n_chunks);
  }
}

// bf16 plans with the "weights in LDS" fused kernel: every weight gradient comes from inr_dw_gemm_bf16.hip
constexpr double kEncCost = 1.5;
static void dw_gemm_bf16_setup(const inr_plan* plan, int64_t nt, inr::DwGemmBf16Args* g, inr::SlabSplit* red) {
  const NetDesc& nd = plan->nd;
  memset(g, 0, sizeof(*g));
  const int D = nd.D;
  int k = 0;
  for (int n0 = 0; n0 < nd.E; n0 += 128) {  // first layer: B = encoder features, 128 frequencies (sine + cosine) a unit
    inr::DwGemmBf16Unit& u = g->unit[k++];
    u.dz_off = w2_stash_G(0, D), u.z_off = -1;
    u.gw_off = nd.L[0].gw_off, u.gb_off = nd.L[0].gb_off, u.M = 256, u.K = nd.L[0].K, u.n0 = n0;
  }
  for (int l = 1; l <= D - 1; ++l) {
    inr::DwGemmBf16Unit& u = g->unit[k++];
    const bool last = l == D - 1;
    u.dz_off = last ? w2_stash_dzl(D) : w2_stash_G(l, D);
    u.z_off = w2_stash_P(l - 1);
    u.gw_off = nd.L[l].gw_off, u.gb_off = nd.L[l].gb_off;
    u.M = last ? nd.L[l].M : 256, u.K = nd.L[l].K, u.n0 = 0;
  }
  g->n_units = k;
  g->TL = W2_TL, g->E = nd.E;
  g->save_floats_per_tile = nd.save_floats_per_tile, g->slab_floats = nd.slab_floats, g->n_tiles = (int)nt;
  // About one workgroup per CU, in two classes (inr_dw_gemm_bf16.h): a first-layer unit costs kEncCost x a hidden unit per
  // tile (65 536 rows, depth 5: 68 us against 54 when each kind runs alone; factors 1.0 / 1.15 / 1.33 / 1.5 / 1.7 measured 72.6 / 70.6 / 69.3 / 66.8 / 67.9 us), so it gets that many times the
  // chunks.  Needs the first layer's weight and bias gradients to be one aligned run of the flat layout (the reduction
  // sums that run over another number of slabs); otherwise one class.
  const int n_enc = (nd.E + 127) / 128, others = k - n_enc;
  const LayerDesc& L0 = nd.L[0];
  const bool run0 = L0.gb_off == L0.gw_off + L0.M * L0.K && (L0.gw_off & 3) == 0 && ((L0.gb_off + L0.M) & 3) == 0;
  if (run0 && !plan->gemm_one_class) {
    const double cost = plan->gemm_enc_cost > 0.0 ? plan->gemm_enc_cost : kEncCost;
    const double per = 256.0 / (cost * n_enc + others);  // chunks of a non-first-layer unit
    g->n_enc_units = n_enc;
    chunk_tiles(nt, (int)(per * cost), &g->tiles_per_chunk_enc, &g->n_chunks_enc);
    chunk_tiles(nt, (256 - n_enc * g->n_chunks_enc) / others, &g->tiles_per_chunk, &g->n_chunks);
  } else {
    g->n_enc_units = n_enc;
    chunk_tiles(nt, 256 / k, &g->tiles_per_chunk, &g->n_chunks);
    g->tiles_per_chunk_enc = g->tiles_per_chunk, g->n_chunks_enc = g->n_chunks;
  }
  // how the reduction reads the chunk slabs
  *red = inr::SlabSplit{0, (nd.P + 3) & ~3, g->n_chunks, 0};  // (a multiple of 4: the fast reduction works on float4)
  if (g->n_chunks_enc != g->n_chunks) red->lo3 = L0.gw_off, red->hi3 = L0.gb_off + L0.M, red->n3 = g->n_chunks_enc;
}

// ---------------------------------------------------------------------------------------------
// How a fused step of a batch-GEMM plan is launched.  With more tiles than workgroups the persistent grid runs whole
// rounds and then a partial one, during which `idle` = n_blocks - (n_tiles mod n_blocks) CUs have nothing to do (WIRE at
// 25 000 rows: 391 tiles of 64 coordinates = 256 + 135; the multiscale config: 1563 = 6 x 256 + 27) -- while the
// weight-gradient GEMM of the tiles already finished only needs their stash.  Split step:
//   main stream:  fused kernel on tiles [0, full)  ->  fused kernel on tiles [full, nt), `rem` workgroups, accumulating
//                 into the slabs of workgroups 0..rem-1  ->  (join)  ->  GEMM part B: tiles [tA, nt)  ->  reduction
//   side stream:  (after the first kernel)  GEMM part A: tiles [0, tA), at most `idle` workgroups
// Part A is sized to end with the partial round: a tile costs the GEMM about kGemmTileShare of the fused kernel's time
// for it on one CU (dW is half of forward + dX, at a slightly better MFMA rate).  Chunk slabs of A, then of B, follow
// the fused kernel's; every sum keeps a fixed order (deterministic), though not the order of the unsplit launch.
// INR_OVERLAP=0 in the environment turns the split off.
// ---------------------------------------------------------------------------------------------
constexpr double kGemmTileShare = 0.4;

// `plain_red`: the reduction of the unsplit GEMM over the whole batch
static void step_schedule(const inr_plan* plan, int64_t nt, int64_t nb, bool overlap, const inr::SlabSplit& plain_red,
                          StepSchedule* sc) {
  sc->split = false;
  sc->full = nt, sc->rem = 0, sc->tA = 0;
  sc->red = plain_red;
  if (!overlap || nt <= nb || nt % nb == 0) return;
  const int64_t rem = nt % nb, full = nt - rem, idle = nb - rem;
  {
    inr::DwGemmArgs probe = plan->gemm;  // (WBM = 0)
    if (idle < inr::dw_gemm_units(probe)) return;  // not even one chunk's workgroups fit beside the partial round
  }
  int64_t tA = (int64_t)(0.9 * (double)idle / kGemmTileShare);
  if (tA > full) tA = full;
  if (tA < nt / 16 || tA < 1) return;  // nothing worth a second launch
  sc->gA = sc->gB = plan->gemm;
  dw_gemm_chunk(sc->gA, 0, tA, (int)idle);
  dw_gemm_chunk(sc->gB, tA, nt, 256);
  sc->split = true;
  sc->full = full, sc->rem = rem, sc->tA = tA;
  sc->red.n2 = sc->gA.n_chunks + sc->gB.n_chunks;
}

// ---------------------------------------------------------------------------------------------
// Row-split fused step: how the 16-coordinate column blocks of a batch are dealt to workgroups.  The stash is read by the
// batch GEMM in whole 128-coordinate slots, so all 8 blocks of every slot are computed (rows past B masked).  `grid`
// workgroups run `rounds` tiles each; tile t has `hi` blocks if t < x, else `lo`; a tile's block count is the kernel's
// NCB, or even (the kernel pairs column blocks: inr_mlp_rs_impl.h rs_active).  Rounds are chosen by cost: a round costs
// its widest tile plus about one block of fixed work (epilogues, barriers, the weight stream's start).
// ---------------------------------------------------------------------------------------------
// Tiles are at most 7 column blocks wide: the kernel keeps 16 NCB accumulators and 16 NCB act' values per lane in AGPRs,
// and at NCB = 8 that is all 256 of them -- the compiler's own AGPR copies then push act' into scratch (measured: the
// forward GEMMs at 88-98 k cycles instead of 71 k).
constexpr int kRsMaxNcb = 7;
static RsSchedule rs_schedule(int64_t nt) {
  const int64_t nblk = 8 * nt;
  RsSchedule s;
  s.grid = (int)std::min<int64_t>(kMaxBlocks, nblk);
  double best = 1e30;
  s.rounds = 1, s.ncb = kRsMaxNcb;
  const int64_t rmax = nblk / s.grid + 1;
  for (int64_t R = 1; R <= rmax; ++R) {
    const int64_t T = s.grid * R, a = nblk / T, rem = nblk % T, ncb = rem ? a + 1 : a;
    if (ncb > kRsMaxNcb || ncb < 1) continue;
    // the busiest workgroup's blocks (workgroup 0: the `hi` tiles come first) + a block's worth of fixed work per round
    const int64_t lo = rem == 0 ? a : (a % 2 == 0 ? a : a - 1), x = rem == 0 ? T : (a % 2 == 0 ? rem : (nblk - (a - 1) * T) / 2);
    const int64_t nhi = std::min<int64_t>(R, (x + s.grid - 1) / s.grid);
    const double cost = (double)(nhi * ncb + (R - nhi) * lo) + 0.9 * (double)R;
    if (cost < best - 1e-9) best = cost, s.rounds = (int)R, s.ncb = (int)ncb;
  }
  const int64_t T = (int64_t)s.grid * s.rounds, a = nblk / T, rem = nblk % T;
  if (rem == 0) {
    s.hi = s.lo = (int)a, s.x = (int)T;
  } else if (a % 2 == 0) {  // NCB = a + 1 odd: full tiles and even ones
    s.hi = (int)a + 1, s.lo = (int)a, s.x = (int)rem;
  } else {                  // NCB = a + 1 even: the others give up a pair
    s.hi = (int)a + 1, s.lo = (int)a - 1, s.x = (int)((nblk - (a - 1) * T) / 2);
  }
  return s;
}

// ---------------------------------------------------------------------------------------------
// Split row-split step.  A single round whose column blocks do not divide by 256 runs the (lo1 + 1)-block kernel on every
// workgroup, `rem` = nblk mod 256 of them on real blocks and the others on a masked one (25 000 rows: 32 tiles of 7, 224
// of 6 -- 30.1 GFLOP issued for 26.3), and the weight-gradient GEMM waits for the widest tile although it needs nothing
// but the stash.  With gradients asked for, the step is launched as
//   main stream:  fused kernel, 256 tiles of lo1 blocks  ->  (fork)  ->  GEMM part A: slots [0, 32 lo1)  ->  (join)  ->
//                 reduction over the grid's slabs, A's chunk slabs, B's chunk slabs
//   side stream:  (fork)  ->  fused kernel on the other `rem` blocks, accumulating into the slabs of workgroups
//                 0 .. n_rem-1  ->  GEMM part B: slots [32 lo1, nt)  ->  (join)
// 256 lo1 blocks end on a slot boundary, so A reads nothing the remainder writes.  A's workgroups + the remainder's are at
// most 256, B's at most the remainder's: each has a CU whatever order the dispatcher picks.  The remainder's tiles are the
// legal shape (k blocks, or an even number below k: rs_active) that the model below likes best; the split runs only
// where that model puts it ahead of the single launch, never under 128 slots (lo1 < 4: the shapes whose step hashes are
// pinned) and never for a schedule of several rounds.  The stash is the single launch's bit for bit; the last layer's
// per-workgroup sums, the loss word and the GEMM's chunk sums group their coordinates differently (fixed order all the same).
//
// The model, in column-block units of the fused kernel (7.9 units = 250 us at the graded shape): a fused launch costs its
// widest tile + 0.9 (rs_schedule); a GEMM launch costs kGemmWgCost + kGemmSlotCost per 128-coordinate slot of its longest
// chunk on 256 x 256 workgroup tiles, half that per slot on the half-height tiles of short chunks (WBM = 2).
// ---------------------------------------------------------------------------------------------
constexpr double kRsRoundFixed = 0.9;
// From the kernel traces of the graded step (profiles/rs_split_before_after.json; under the tracer the 7-block launch
// takes 270.5 us, 1 unit = 34.2 us): dw_gemm_split_kernel in chunks of 9 half-height slots (part A) 88.0 us = 2.57 units,
// of 2 (part B) 25.1 us = 0.73, of 8 (the whole batch, 250 workgroups) 85.1 us = 2.49.  A and B give 0.53 a slot and
// 0.21 a launch; the whole-batch launch sits 0.18 above that line, so the fixed share is set between them.
// Calibrated on that one plan (depth 5, gauss-256) and on nothing else: at another depth a column block of the fused
// kernel is cheaper or dearer while these constants stay, so the unit drifts.  No other depth was measured.  The drift is
// towards NOT splitting where the network is shallower (a depth-3 plan never engages: the model, not a measurement, says
// its GEMM is shorter than a remainder launch), and such plans simply keep the single launch they had.
constexpr double kGemmWgCost = 0.25;
constexpr double kGemmSlotCost = 0.53;

static double dw_gemm_model(const inr::DwGemmArgs& g) {
  return kGemmWgCost + kGemmSlotCost * (double)g.tiles_per_chunk * (g.WBM == 2 ? 0.5 : 1.0);
}

// `gemm`: the plan's GEMM (no tiles or chunks yet); `one`, `plain`, `plain_red`: the single launch, its GEMM, its reduction
static void rs_split_schedule(const inr::DwGemmArgs& gemm, int64_t nt, const RsSchedule& one, const inr::DwGemmArgs& plain,
                              const inr::SlabSplit& plain_red, RsSplit* sp) {
  sp->split = false;
  sp->lo1 = sp->blk0 = 0;
  sp->red = plain_red;
  const int64_t nblk = 8 * nt, lo1 = nblk / kMaxBlocks, rem = nblk % kMaxBlocks;
  if (one.grid != kMaxBlocks || one.rounds != 1 || rem == 0 || lo1 < 4) return;
  const int64_t slotsA = lo1 * kMaxBlocks / 8;
  double best = (double)one.ncb + kRsRoundFixed + dw_gemm_model(plain);  // the single launch + its GEMM
  for (int k = 1; k <= kRsMaxNcb; ++k) {
    for (int lo = 0; lo < k; lo += 2) {  // x tiles of k blocks, then y of `lo` (0: none), as few tiles as there can be
      int64_t x = -1, y = 0;
      if (lo == 0) {
        if (rem % k == 0) x = rem / k;
      } else {
        for (y = 1; y < k && y * lo < rem; ++y)
          if ((rem - y * lo) % k == 0) {
            x = (rem - y * lo) / k;
            break;
          }
      }
      if (x < 1) continue;
      const int64_t n_rem = x + y;
      if (n_rem >= kMaxBlocks) continue;
      inr::DwGemmArgs gA = gemm, gB = gemm;
      dw_gemm_chunk(gA, 0, slotsA, (int)(kMaxBlocks - n_rem));
      dw_gemm_chunk(gB, slotsA, nt, (int)n_rem);
      if ((int64_t)gA.n_chunks * inr::dw_gemm_units(gA) > kMaxBlocks - n_rem) continue;
      if ((int64_t)gB.n_chunks * inr::dw_gemm_units(gB) > n_rem) continue;
      const double t = (double)lo1 + kRsRoundFixed +
                       std::max(dw_gemm_model(gA), (double)k + kRsRoundFixed + dw_gemm_model(gB));
      if (!(t < best - 1e-9)) continue;
      best = t;
      sp->split = true;
      sp->lo1 = (int)lo1, sp->blk0 = (int)(lo1 * kMaxBlocks);
      sp->first = RsSchedule{kMaxBlocks, 1, (int)lo1, (int)lo1, (int)lo1, kMaxBlocks};
      sp->rest = RsSchedule{(int)n_rem, 1, k, k, lo == 0 ? k : lo, (int)x};
      sp->gA = gA, sp->gB = gB;
      sp->red.n2 = gA.n_chunks + gB.n_chunks;
    }
  }
}

// Which fused kernel runs a batch of nt 128-coordinate slots?  The row-split kernel, unless inr_mlp_kernel's rounds of 256
// tiles are (all but) full: then both do the same MFMA work and the row-split kernel only adds a round (65 536 rows:
// 6 + 6 + 4 column blocks per workgroup, 649 us against 629 us; 25 000 rows: 266 us against 316 us).
// INR_RS=0 / 1 in the environment (`e`) forces one or the other.
static bool rs_enabled(const char* e, int64_t nt) {
  if (e != nullptr && e[0] == '0') return false;
  if (e != nullptr && e[0] == '1') return true;
  const int64_t rounds = (nt + kMaxBlocks - 1) / kMaxBlocks;
  return (double)nt < 0.97 * (double)(rounds * kMaxBlocks);
}

// B >= 1.  INR_RS and INR_OVERLAP are read here, per call: tests flip them between calls on one plan in one process
void call_layout(const inr_plan* plan, int64_t B, CallLayout* c) {
  const NetDesc& nd = plan->nd;
  const char* e_rs = getenv("INR_RS");
  const char* e_overlap = getenv("INR_OVERLAP");
  const int tl = 32 * nd.NW;
  const int64_t nt = c->nt = (B + tl - 1) / tl;
  c->nb = nt < kMaxBlocks ? nt : kMaxBlocks;
  if (nd.bf16) {  // the bf16 kernel's workgroups take two 128-coordinate tiles each
    const int64_t wt = nt > kMaxBlocks ? (nt + 1) / 2 : nt;  // (one each while that fills fewer CUs)
    c->nb = wt < kMaxBlocks ? wt : kMaxBlocks;
  }
  // fused steps of batch-GEMM plans stash per TILE (n_tiles slots): the GEMM reads the whole batch's stash
  c->save_slots = plan->dw_route != 0 ? nt : c->nb;
  c->n_slabs = c->nb;
  c->rs = false;
  c->step.split = false;
  c->rsplit.split = false, c->rs_split = false;
  if (plan->dw_route == 2) {  // (the unfused backward of these plans needs nb slabs only: covered)
    dw_gemm_bf16_setup(plan, nt, &c->bf16, &c->bf16_red);
    c->n_slabs = c->nb + std::max(c->bf16.n_chunks, c->bf16.n_chunks_enc);
  } else if (plan->dw_route == 1) {
    c->plain = plan->gemm;
    dw_gemm_chunk(c->plain, 0, nt, 256);
    c->plain_red = plan->gemm_cover;
    c->plain_red.n2 = c->plain.n_chunks;
    // (a split step has its own chunking; the unfused backward keeps the plain one)
    const bool overlap = !(e_overlap != nullptr && e_overlap[0] == '0');
    step_schedule(plan, nt, c->nb, overlap, c->plain_red, &c->step);
    // (row-split fused steps run rs_schedule's grid -- more workgroups than tiles while the batch is under 256 slots; the
    // workspace follows neither INR_RS nor INR_OVERLAP: it covers both fused kernels' grids and every chunking)
    int64_t grid = c->nb;
    int split_chunks = 0;
    if (nd.rs) {
      c->rsched = rs_schedule(nt);
      c->rs = rs_enabled(e_rs, nt);
      grid = std::max<int64_t>(grid, c->rsched.grid);
      rs_split_schedule(plan->gemm, nt, c->rsched, c->plain, c->plain_red, &c->rsplit);
      c->rs_split = c->rs && overlap && c->rsplit.split;
      if (c->rsplit.split) split_chunks = c->rsplit.red.n2;
    }
    c->n_slabs = grid + std::max(std::max(c->plain.n_chunks, c->step.red.n2), split_chunks);
  }
}

// ---- weight-image sets: which are valid after an event, which a call reads (no state here: inr_host.h) ----
int image_sets_after(int valid, int event, int sets) {
  sets &= inr::IMG_ALL;
  if (event == IMG_EV_UPDATE) return sets;  // the parameters moved: what the update did not write is stale
  return (valid | sets) & inr::IMG_ALL;     // a pack, or the re-pack in front of a read
}

int image_sets_read(int call, bool row_split) {
  if (call == IMG_CALL_FORWARD) return inr::IMG_FWD;
  if (call == IMG_CALL_BACKWARD) return inr::IMG_FWD | inr::IMG_TR;  // (inr_mlp_kernel stages the last layer's forward image in every mode)
  return row_split ? inr::IMG_RS : (inr::IMG_FWD | inr::IMG_TR);
}

bool lazy_pack_enabled() {
  const char* e = getenv("INR_LAZY_PACK");
  return e != nullptr && e[0] == '1';  // opt-in: see DESIGN 4.2 (a recorded hash of `packed` after a step holds every set)
}

// B and, from it, the call's layout: the one place an entry learns its tiles, grids, chunks and workspace
int begin_call(const inr_plan* plan, int64_t B, const char* who, CallLayout* c) {
  if (B <= 0) return fail(INR_ERR_INVALID, "%s: B = %lld", who, (long long)B);
  call_layout(plan, B, c);
  return INR_OK;
}

extern "C" {

// (the three older readers of a call's layout report a bad B in inr_plan_launch_dims' name; inr_plan_step_split in its own)
int inr_plan_workspace(const inr_plan* plan, int64_t B, int64_t* step_save_slots, int64_t* n_slabs) {
  if (plan == nullptr || step_save_slots == nullptr || n_slabs == nullptr)
    return fail(INR_ERR_INVALID, "inr_plan_workspace: null argument");
  CallLayout c;
  if (int rc = begin_call(plan, B, "inr_plan_launch_dims", &c)) return rc;
  *step_save_slots = c.save_slots, *n_slabs = c.n_slabs;
  return INR_OK;
}

int inr_plan_step_info(const inr_plan* plan, int64_t B, inr_step_info* out) {
  if (plan == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_plan_step_info: null argument");
  CallLayout c;
  if (int rc = begin_call(plan, B, "inr_plan_launch_dims", &c)) return rc;
  memset(out, 0, sizeof(*out));
  out->hidden_blocks = plan->nd.NB;
  if (c.rs) {
    const RsSchedule& s = c.rsched;
    out->row_split = 1, out->ncb = s.ncb, out->grid = s.grid, out->rounds = s.rounds;
    out->hi = s.hi, out->lo = s.lo, out->n_hi = s.x;
  } else {
    out->grid = (int32_t)c.nb, out->rounds = (int32_t)((c.nt + c.nb - 1) / c.nb);
  }
  return INR_OK;
}

int inr_plan_step_split(const inr_plan* plan, int64_t B, int64_t* out) {
  if (plan == nullptr || out == nullptr) return fail(INR_ERR_INVALID, "inr_plan_step_split: null argument");
  CallLayout c;
  if (int rc = begin_call(plan, B, "inr_plan_step_split", &c)) return rc;
  for (int i = 0; i < INR_STEP_SPLIT_WORDS; ++i) out[i] = 0;
  out[15] = c.n_slabs;
  if (!c.rs_split) return INR_OK;
  const RsSplit& sp = c.rsplit;
  inr::DwGemmArgs gA = sp.gA, gB = sp.gB;
  out[0] = 1, out[1] = sp.lo1;
  out[2] = sp.rest.hi, out[3] = sp.rest.lo, out[4] = sp.rest.x, out[5] = sp.rest.grid, out[6] = sp.rest.ncb;
  out[7] = gA.n_tiles, out[8] = gA.tiles_per_chunk, out[9] = gA.n_chunks, out[10] = gA.n_chunks * inr::dw_gemm_units(gA);
  out[11] = gB.tile0, out[12] = gB.tiles_per_chunk, out[13] = gB.n_chunks, out[14] = gB.n_chunks * inr::dw_gemm_units(gB);
  return INR_OK;
}

int inr_image_sets_after(int32_t valid, int32_t event, int32_t sets) { return image_sets_after(valid, event, sets); }

int inr_image_sets_read(int32_t call, int32_t row_split) { return image_sets_read(call, row_split != 0); }

int inr_plan_image_sets(const inr_plan* plan, int32_t* valid, int32_t* lazy) {
  if (plan == nullptr || valid == nullptr || lazy == nullptr)
    return fail(INR_ERR_INVALID, "inr_plan_image_sets: null argument");
  *valid = plan->img_valid;
  *lazy = plan->nd.rs && !plan->img_eager && lazy_pack_enabled() ? 1 : 0;
  return INR_OK;
}

int inr_plan_launch_dims(const inr_plan* plan, int64_t B, int64_t* n_tiles, int64_t* n_blocks) {
  if (plan == nullptr || n_tiles == nullptr || n_blocks == nullptr)
    return fail(INR_ERR_INVALID, "inr_plan_launch_dims: null argument");
  CallLayout c;
  if (int rc = begin_call(plan, B, "inr_plan_launch_dims", &c)) return rc;
  *n_tiles = c.nt, *n_blocks = c.nb;
  return INR_OK;
}

}  // extern "C"
