// inr_api.hip -- the network entries of the C-ABI of libinr_mi355x.so (see include/inr_abi.h): forward, backward and
// fused step.  Plain pointers and sizes only; validates arguments up front; never allocates device memory; never syncs.
#include <cstring>
#include <mutex>
#include <string>

#include "inr_host.h"

#ifdef INR_STAMPS
namespace inr {
long long* g_stamp_buf = nullptr;
long long g_stamp_cap = 0;
}  // namespace inr
using inr::g_stamp_buf;
using inr::g_stamp_cap;
#endif

extern "C" {

// `blk0`, `accumulate`: the remainder launch of a split step (behind the first launch's blocks, adding to its slabs)
static int launch_rs(const inr_plan* plan, const LossDesc& ld, inr::MlpArgs a, int64_t nt, const RsSchedule& sc,
                     hipStream_t st, int blk0 = 0, int accumulate = 0) {
  a.n_tiles = (int)nt;
  a.rs_hi = sc.hi, a.rs_lo = sc.lo, a.rs_x = sc.x, a.rs_rounds = sc.rounds;
  a.tile0 = 0, a.accumulate = accumulate, a.rs_blk0 = blk0;
  return hip_done(inr::rs_kernel(sc.ncb)(plan->nd, ld, a, sc.grid, st), "inr row-split kernel launch");
}

static hipStream_t side_stream(const inr_plan* plan) {
  std::lock_guard<std::mutex> lock(plan->side_mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  if (plan->side != nullptr && plan->side_dev != dev) {
    (void)hipStreamDestroy(plan->side);
    if (plan->fork != nullptr) (void)hipEventDestroy(plan->fork);
    if (plan->join != nullptr) (void)hipEventDestroy(plan->join);
    plan->side = nullptr;
    plan->fork = plan->join = nullptr;
  }
  if (plan->side == nullptr) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&plan->side, hipStreamNonBlocking, least) != hipSuccess) plan->side = nullptr;
    if (plan->side != nullptr && (hipEventCreateWithFlags(&plan->fork, hipEventDisableTiming) != hipSuccess ||
                                  hipEventCreateWithFlags(&plan->join, hipEventDisableTiming) != hipSuccess)) {
      if (plan->fork != nullptr) (void)hipEventDestroy(plan->fork);
      (void)hipStreamDestroy(plan->side);
      plan->side = nullptr;
      plan->fork = plan->join = nullptr;
    }
    plan->side_dev = dev;
  }
  return plan->side;
}

// a call's scratch against what the plan needs: `save_slots` stash slots (0: none), `n_slabs` slabs (0: none)
static int check_ws(const inr_plan* plan, const inr_workspace* ws, int64_t save_slots, int64_t n_slabs,
                    const char* who) {
  if (ws == nullptr) return fail(INR_ERR_INVALID, "%s: null workspace", who);
  const int64_t need_save = save_slots * (int64_t)plan->nd.save_floats_per_tile;
  const int64_t need_slabs = n_slabs * (int64_t)plan->nd.slab_floats;
  if (save_slots > 0 && (ws->save == nullptr || ws->save_floats < need_save))
    return fail(INR_ERR_INVALID, "%s: stash of %lld floats, the call needs %lld (%lld slots of %d; see "
                "inr_plan_workspace)", who, (long long)(ws->save == nullptr ? 0 : ws->save_floats),
                (long long)need_save, (long long)save_slots, plan->nd.save_floats_per_tile);
  if (n_slabs > 0 && (ws->slabs == nullptr || ws->slab_floats < need_slabs))
    return fail(INR_ERR_INVALID, "%s: %lld slab floats, the call needs %lld (%lld slabs of %d; see "
                "inr_plan_workspace)", who, (long long)(ws->slabs == nullptr ? 0 : ws->slab_floats),
                (long long)need_slabs, (long long)n_slabs, plan->nd.slab_floats);
  return INR_OK;
}

static int launch(const inr_plan* plan, const LossDesc& ld, const inr::MlpArgs& a, int mode, int grid,
                  hipStream_t st) {
  return hip_done(inr::net_kernel(plan->nd)(plan->nd, ld, a, mode, grid, st), "inr mlp kernel launch");
}

// Row-split plans: the image sets this call's kernel reads must hold the current parameters.  What an earlier lazy update
// left stale (inr_host.h: img_valid) is re-packed here, on the call's stream, in front of the kernel -- `packed` is the
// caller's buffer, const to the kernels, rewritten with what a full pack would have put there.
static int ensure_images(const inr_plan* plan, const float* params, const float* packed, int reads, hipStream_t st,
                         const char* who) {
  const int stale = plan->nd.rs ? reads & ~plan->img_valid : 0;
  if (stale == 0) return INR_OK;
  inr::AdamArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.skip_sets = inr::IMG_ALL & ~stale;
  hipError_t e = inr::launch_adam_pack(plan->nd, const_cast<float*>(params), nullptr, nullptr, nullptr,
                                       const_cast<float*>(packed), aa, st);
  if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": re-pack of stale weight images").c_str());
  images_note(plan, IMG_EV_READ, stale, st);
  return INR_OK;
}

// ---- the six network calls: one prologue ----
// Null pointers, the plan's family and what its input needs, in the order every entry has always reported them: plain
// entries name the family first, the _multi ones the inputs (`need_dist`: forward / backward of a bounded model).
static int check_net_call(const char* who, bool null_arg, const inr_plan* plan, bool multi, const float* enc_B,
                          bool need_dist, const float* dist) {
  if (null_arg) return fail(INR_ERR_INVALID, "%s: null argument", who);
  if (!multi && plan->nd.mfn_n > 0) return fail(INR_ERR_INVALID, "%s: multiplicative-filter plans use %s_multi", who, who);
  if (plan->nd.input == IN_GAUSS && enc_B == nullptr) return fail(INR_ERR_INVALID, "%s: enc_B is null", who);
  if (need_dist && plan->nd.bounded && dist == nullptr) return fail(INR_ERR_INVALID, "%s: bounded model needs dist", who);
  if (multi && plan->nd.mfn_n == 0) return fail(INR_ERR_INVALID, "%s: not a multiplicative-filter plan", who);
  return INR_OK;
}

static int check_step_loss(const char* who, const inr_plan* plan, const inr_loss_desc* loss) {
  if (loss->kind < INR_LOSS_L2_HALF || loss->kind > INR_LOSS_CENTER)
    return fail(INR_ERR_INVALID, "%s: loss kind %d", who, loss->kind);
  if (loss->kind >= INR_LOSS_LOGSPACE && plan->nd.out_f != 2)
    return fail(INR_ERR_INVALID, "%s: complex-row losses need out_features == 2", who);
  return INR_OK;
}

// kernel arguments every network call shares; the entry adds its outputs / targets
static inr::MlpArgs net_args(const float* params, const float* packed, const float* x, const float* enc_B, int64_t B,
                             const CallLayout& c, const inr_workspace* ws) {
  inr::MlpArgs a;
  memset(&a, 0, sizeof(a));
  a.params = params;
  a.packed = packed;
  a.x = x;
  a.encB = enc_B;
  a.B = B;
  a.n_tiles = (int)c.nt;
  if (ws != nullptr) a.save = ws->save;
  return a;
}

// ... and those of a fused step (mode 2): slabs, the plan's weight-gradient route, per-tile or per-workgroup stash
static int step_args(const inr_plan* plan, const inr_workspace* ws, const char* who, inr::MlpArgs* a) {
  a->slabs = ws->slabs;
  a->dw_gemm = plan->dw_route;
  a->save_by_block = a->dw_gemm ? 0 : 1;
  if (a->dw_gemm == 2) {
    a->dz_state = dz_state_alloc(plan);
    if (a->dz_state == nullptr) return fail(INR_ERR_HIP, "%s: no gradient-scale state on this device", who);
  }
#ifdef INR_STAMPS
  a->dbg = g_stamp_buf;
  a->dbg_cap = g_stamp_cap;
#endif
  return INR_OK;
}

int inr_forward(const inr_plan* plan, const float* params, const float* packed, const float* x,
                const float* enc_B, int64_t B, float* out, const inr_workspace* ws, void* stream) {
  const char* who = "inr_forward";
  const bool null_arg = plan == nullptr || params == nullptr || packed == nullptr || x == nullptr || out == nullptr;
  if (int rc = check_net_call(who, null_arg, plan, false, enc_B, false, nullptr)) return rc;
  const bool saving = ws != nullptr && ws->save != nullptr;
  if (plan->nd.hact == ACT_GABOR2D && !saving)
    return fail(INR_ERR_INVALID, "inr_forward: WIRE2D plans need a save buffer (n_tiles * save_floats_per_tile floats)");
  CallLayout c;
  if (int rc = begin_call(plan, B, who, &c)) return rc;
  if (saving)
    if (int rc = check_ws(plan, ws, c.nt, 0, who)) return rc;
  if (int rc = ensure_images(plan, params, packed, image_sets_read(IMG_CALL_FORWARD, false), (hipStream_t)stream, who))
    return rc;
  inr::MlpArgs a = net_args(params, packed, x, enc_B, B, c, ws);
  a.out = out;
  a.save_by_block = 0;
  LossDesc ld;
  memset(&ld, 0, sizeof(ld));
  return launch(plan, ld, a, 0, (int)c.nb, (hipStream_t)stream);
}

// the Adam update folded into the slab reduction's launch (inr_train_adam_step)
struct AdamFuse {
  float *params, *m1, *m2, *packed;
  inr::AdamArgs aa;
};

static hipError_t reduce_stage(const inr_plan* plan, const float* slabs, int nb, float* grads, float* loss_out,
                               const float* params, const float* packed, hipStream_t st, const inr::SlabSplit& split,
                               const AdamFuse* af) {
  if (af != nullptr)
    return inr::launch_reduce_slabs_adam(plan->nd, slabs, nb, grads, loss_out, af->params, af->m1, af->m2, af->packed,
                                         af->aa, st, split);
  return inr::launch_reduce_slabs(plan->nd, slabs, nb, grads, loss_out, params, packed, st, split);
}

// dW GEMM over the whole batch (plans that use it), its chunk slabs behind the `nb` workgroup slabs of the kernel that
// ran, + deterministic slab reduction into flat gradients
static int finish_gradients(const inr_plan* plan, const inr::MlpArgs& a, const CallLayout& c, int64_t nb, float* grads,
                            float* loss_out, const float* params, const float* packed, hipStream_t st,
                            const char* who, const AdamFuse* af = nullptr) {
  inr::SlabSplit split{0, 0, 0, 0};
  if (a.dw_gemm == 2) {  // bf16 fused step: all of dW / db from the bf16 batch GEMM, summed over its chunk slabs
    inr::DwGemmBf16Args g = c.bf16;
    g.save = a.save;
    g.slabs = a.slabs + (size_t)nb * plan->nd.slab_floats;
    g.coords = a.x;
    g.encB = a.encB;
    g.B = a.B;
    g.dz_state = a.dz_state + (a.dout != nullptr ? 4 : 0);  // split steps keep their own scale
    g.dz_count = a.dz_state + 8 + (a.dout != nullptr ? 2 : 0);
    hipError_t e = inr::launch_dw_gemm_bf16(g, st);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": bf16 weight-gradient GEMM").c_str());
    split = c.bf16_red;
  } else if (a.dw_gemm) {
    inr::DwGemmArgs g = c.plain;
    g.save = a.save;
    g.slabs = a.slabs + (size_t)nb * plan->nd.slab_floats;
    hipError_t e = inr::launch_dw_gemm(g, st);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": weight-gradient GEMM").c_str());
    split = c.plain_red;
  }
  hipError_t e = reduce_stage(plan, a.slabs, (int)nb, grads, loss_out, params, packed, st, split, af);
  if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": slab reduction").c_str());
  return INR_OK;
}

int inr_backward(const inr_plan* plan, const float* params, const float* packed, const float* x,
                 const float* enc_B, int64_t B, const float* dout, const inr_workspace* ws,
                 float* grads, void* stream) {
  const char* who = "inr_backward";
  const bool null_arg = plan == nullptr || params == nullptr || packed == nullptr || x == nullptr || dout == nullptr ||
                        ws == nullptr || grads == nullptr;
  if (int rc = check_net_call(who, null_arg, plan, false, enc_B, false, nullptr)) return rc;
  CallLayout c;
  if (int rc = begin_call(plan, B, who, &c)) return rc;
  if (int rc = check_ws(plan, ws, c.nt, c.n_slabs, who)) return rc;
  if (int rc = ensure_images(plan, params, packed, image_sets_read(IMG_CALL_BACKWARD, false), (hipStream_t)stream, who))
    return rc;
  inr::MlpArgs a = net_args(params, packed, x, enc_B, B, c, ws);
  a.dout = dout;
  a.slabs = ws->slabs;
  a.save_by_block = 0;
  a.dw_gemm = plan->dw_route;
  LossDesc ld;
  memset(&ld, 0, sizeof(ld));
  if (a.dw_gemm == 2) {
    a.dz_state = dz_state_alloc(plan);
    if (a.dz_state == nullptr) return fail(INR_ERR_HIP, "inr_backward: no gradient-scale state on this device");
    if (dz_needs_calibration(plan, 1, B, 0)) {  // a pass for the scale (the forward half's stash is not touched)
      int rc = launch(plan, ld, a, 1, (int)c.nb, (hipStream_t)stream);
      if (rc != INR_OK) return rc;
      hipError_t e = inr::launch_dz_roll(a.dz_state + 4, nullptr, (hipStream_t)stream);
      if (e != hipSuccess) return hip_fail(e, "inr_backward: gradient-scale calibration");
    }
  }
  int rc = launch(plan, ld, a, 1, (int)c.nb, (hipStream_t)stream);
  if (rc != INR_OK) return rc;
  if (a.dw_gemm == 2) dz_mark(plan, 1, B, 0);
  return finish_gradients(plan, a, c, c.nb, grads, nullptr, params, packed, (hipStream_t)stream, who);
}

// fused step (mode 2) + weight gradients + reduction, split over two streams where the layout's StepSchedule says so
static int run_fused_step(const inr_plan* plan, const LossDesc& ld, const inr::MlpArgs& a, const CallLayout& c,
                          float* grads, float* loss_out, const float* params, const float* packed, hipStream_t st,
                          const char* who, const AdamFuse* af = nullptr) {
  const int64_t nb = c.nb;
  if (c.rs) {
    // row-split kernel.  One launch of whole rounds, then the batch GEMM and the reduction over its grid's slabs: calls
    // without gradients (profiling), calls inside a graph capture (a captured graph keeps one branch) and every batch
    // whose layout has no split
    hipStream_t side = nullptr;
    if (grads != nullptr && c.rs_split && !stream_capturing(st)) side = side_stream(plan);
    if (side == nullptr) {
      int rc = launch_rs(plan, ld, a, c.nt, c.rsched, st);
      if (rc != INR_OK) return rc;
      if (grads == nullptr) return INR_OK;
      return finish_gradients(plan, a, c, c.rsched.grid, grads, loss_out, params, packed, st, who, af);
    }
    // split (inr_layout.hip rs_split_schedule): the narrower round, then GEMM part A here beside the remainder launch and
    // GEMM part B (which needs the remainder's slots only) on the side stream
    const RsSplit& sp = c.rsplit;
    const hipEvent_t fork = plan->fork, join = plan->join;
    float* chunk_slabs = a.slabs + (size_t)sp.first.grid * plan->nd.slab_floats;
    inr::DwGemmArgs gA = sp.gA, gB = sp.gB;
    gA.save = gB.save = a.save;
    gA.slabs = chunk_slabs;
    gB.slabs = chunk_slabs + (size_t)gA.n_chunks * plan->nd.slab_floats;
    int rc = launch_rs(plan, ld, a, c.nt, sp.first, st);
    hipError_t e = hipSuccess;
    if (rc == INR_OK) e = hipEventRecord(fork, st);
    if (rc == INR_OK && e == hipSuccess) e = hipStreamWaitEvent(side, fork, 0);
    // (the remainder is queued before part A: the longer branch.  Queued the other way round, or with the branches' streams
    // exchanged, the step takes the same time within 1 us: profiles/rs_split_before_after.json)
    if (rc == INR_OK && e == hipSuccess) rc = launch_rs(plan, ld, a, c.nt, sp.rest, side, sp.blk0, 1);
    if (rc == INR_OK && e == hipSuccess) e = inr::launch_dw_gemm(gA, st);
    if (rc == INR_OK && e == hipSuccess) e = inr::launch_dw_gemm(gB, side);
    if (rc == INR_OK && e == hipSuccess) e = hipEventRecord(join, side);
    if (rc == INR_OK && e == hipSuccess) e = hipStreamWaitEvent(st, join, 0);
    if (rc == INR_OK && e == hipSuccess)
      e = reduce_stage(plan, a.slabs, sp.first.grid, grads, loss_out, params, packed, st, sp.red, af);
    if (rc != INR_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": split row-split step").c_str());
    return INR_OK;
  }
  const StepSchedule& sc = c.step;
  hipStream_t side = nullptr;
  if (grads != nullptr && sc.split) side = side_stream(plan);
  if (a.dw_gemm == 2 && dz_needs_calibration(plan, 0, a.B, ld.kind)) {  // bf16: a pass of the kernel for the scale
    int rc = launch(plan, ld, a, 2, (int)nb, st);
    if (rc != INR_OK) return rc;
    hipError_t e = inr::launch_dz_roll(a.dz_state, nullptr, st);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": gradient-scale calibration").c_str());
  }
  if (side == nullptr) {
    int rc = launch(plan, ld, a, 2, (int)nb, st);
    if (rc != INR_OK) return rc;
    if (a.dw_gemm == 2) dz_mark(plan, 0, a.B, ld.kind);
    if (grads == nullptr) return INR_OK;  // profiling: leave the per-block slabs unreduced
    return finish_gradients(plan, a, c, nb, grads, loss_out, params, packed, st, who, af);
  }
  const hipEvent_t fork = plan->fork, join = plan->join;  // (created once, with the side stream)
  float* chunk_slabs = a.slabs + (size_t)nb * plan->nd.slab_floats;
  inr::MlpArgs a1 = a, a2 = a;
  a1.n_tiles = (int)sc.full;
  a2.tile0 = (int)sc.full, a2.accumulate = 1;
  inr::DwGemmArgs gA = sc.gA, gB = sc.gB;
  gA.save = gB.save = a.save;
  gA.slabs = chunk_slabs;
  gB.slabs = chunk_slabs + (size_t)gA.n_chunks * plan->nd.slab_floats;
  int rc = launch(plan, ld, a1, 2, (int)nb, st);
  hipError_t e = hipSuccess;
  if (rc == INR_OK) e = hipEventRecord(fork, st);
  if (rc == INR_OK && e == hipSuccess) rc = launch(plan, ld, a2, 2, (int)sc.rem, st);  // (queued before the GEMM: the critical path)
  if (rc == INR_OK && e == hipSuccess) e = hipStreamWaitEvent(side, fork, 0);
  if (rc == INR_OK && e == hipSuccess) e = inr::launch_dw_gemm(gA, side);
  if (rc == INR_OK && e == hipSuccess) e = hipEventRecord(join, side);
  if (rc == INR_OK && e == hipSuccess) e = hipStreamWaitEvent(st, join, 0);
  if (rc == INR_OK && e == hipSuccess) e = inr::launch_dw_gemm(gB, st);
  if (rc == INR_OK && e == hipSuccess)
    e = reduce_stage(plan, a.slabs, (int)nb, grads, loss_out, params, packed, st, sc.red, af);
  if (rc != INR_OK) return rc;
  if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": split step").c_str());
  return INR_OK;
}

static int train_step_impl(const inr_plan* plan, const inr_loss_desc* loss, const float* params, const float* packed,
                           const float* x, const float* enc_B, const float* gt, const uint8_t* mask, int64_t B,
                           const inr_workspace* ws, float* grads, float* loss_out, void* stream, const AdamFuse* af) {
  const char* who = "inr_train_step";
  const bool null_arg = plan == nullptr || loss == nullptr || params == nullptr || packed == nullptr || x == nullptr ||
                        gt == nullptr || ws == nullptr || loss_out == nullptr;
  if (int rc = check_net_call(who, null_arg, plan, false, enc_B, false, nullptr)) return rc;
  if (int rc = check_step_loss(who, plan, loss)) return rc;
  CallLayout c;
  if (int rc = begin_call(plan, B, who, &c)) return rc;
  if (int rc = check_ws(plan, ws, c.save_slots, c.n_slabs, who)) return rc;
  const int reads = image_sets_read(IMG_CALL_STEP, c.rs);
  if (int rc = ensure_images(plan, params, packed, reads, (hipStream_t)stream, who)) return rc;
  inr::MlpArgs a = net_args(params, packed, x, enc_B, B, c, ws);
  a.gt = gt;
  a.mask = mask;
  if (int rc = step_args(plan, ws, who, &a)) return rc;
  LossDesc ld;
  to_loss_desc(loss, &ld);
  if (af == nullptr || grads == nullptr)
    return run_fused_step(plan, ld, a, c, grads, loss_out, params, packed, (hipStream_t)stream, who, af);
  // the update writes the images this step's kernel read -- the ones the next step will read -- and leaves the rest stale
  AdamFuse lazy = *af;
  lazy.aa.skip_sets = image_sets_skip(plan, reads, (hipStream_t)stream);
  int rc = run_fused_step(plan, ld, a, c, grads, loss_out, params, packed, (hipStream_t)stream, who, &lazy);
  if (rc == INR_OK) images_note(plan, IMG_EV_UPDATE, inr::IMG_ALL & ~lazy.aa.skip_sets, (hipStream_t)stream);
  return rc;
}

int inr_train_step(const inr_plan* plan, const inr_loss_desc* loss, const float* params, const float* packed,
                   const float* x, const float* enc_B, const float* gt, const uint8_t* mask, int64_t B,
                   const inr_workspace* ws, float* grads, float* loss_out, void* stream) {
  return train_step_impl(plan, loss, params, packed, x, enc_B, gt, mask, B, ws, grads, loss_out, stream, nullptr);
}

int inr_forward_multi(const inr_plan* plan, const float* params, const float* packed, const float* coords,
                      const float* enc_B, const float* dist, int64_t B, float* out, const inr_workspace* ws,
                      int32_t by_block, void* stream) {
  const char* who = "inr_forward_multi";
  const bool null_arg = plan == nullptr || params == nullptr || packed == nullptr || coords == nullptr || out == nullptr ||
                        ws == nullptr;
  if (int rc = check_net_call(who, null_arg, plan, true, enc_B, true, dist)) return rc;
  CallLayout c;
  if (int rc = begin_call(plan, B, who, &c)) return rc;
  if (int rc = check_ws(plan, ws, by_block ? c.nb : c.nt, 0, who)) return rc;
  inr::MlpArgs a = net_args(params, packed, coords, enc_B, B, c, ws);
  a.out = out;
  a.dist = dist;
  a.save_by_block = by_block ? 1 : 0;
  LossDesc ld;
  memset(&ld, 0, sizeof(ld));
  return launch(plan, ld, a, 0, (int)c.nb, (hipStream_t)stream);
}

int inr_backward_multi(const inr_plan* plan, const float* params, const float* packed, const float* coords,
                       const float* enc_B, const float* dist, int64_t B, const float* dout,
                       const inr_workspace* ws, float* grads, void* stream) {
  const char* who = "inr_backward_multi";
  const bool null_arg = plan == nullptr || params == nullptr || packed == nullptr || coords == nullptr || dout == nullptr ||
                        ws == nullptr || grads == nullptr;
  if (int rc = check_net_call(who, null_arg, plan, true, enc_B, true, dist)) return rc;
  CallLayout c;
  if (int rc = begin_call(plan, B, who, &c)) return rc;
  if (int rc = check_ws(plan, ws, c.nt, c.n_slabs, who)) return rc;
  inr::MlpArgs a = net_args(params, packed, coords, enc_B, B, c, ws);
  a.dout = dout;
  a.dist = dist;
  a.slabs = ws->slabs;
  a.save_by_block = 0;
  a.dw_gemm = plan->dw_route;
  LossDesc ld;
  memset(&ld, 0, sizeof(ld));
  int rc = launch(plan, ld, a, 1, (int)c.nb, (hipStream_t)stream);
  if (rc != INR_OK) return rc;
  return finish_gradients(plan, a, c, c.nb, grads, nullptr, params, packed, (hipStream_t)stream, who);
}

int inr_train_step_multi(const inr_plan* plan, const inr_loss_desc* loss, const float* params, const float* packed,
                         const float* coords, const float* enc_B, const float* gt, const float* dist,
                         const uint8_t* mask, int64_t B, const inr_workspace* ws, float* grads, float* loss_out,
                         void* stream) {
  const char* who = "inr_train_step_multi";
  const bool null_arg = plan == nullptr || loss == nullptr || params == nullptr || packed == nullptr || coords == nullptr ||
                        gt == nullptr || ws == nullptr || loss_out == nullptr;
  if (int rc = check_net_call(who, null_arg, plan, true, enc_B, false, nullptr)) return rc;
  if (int rc = check_step_loss(who, plan, loss)) return rc;
  if ((loss->cons_w != 0.f || plan->nd.bounded) && dist == nullptr)
    return fail(INR_ERR_INVALID, "inr_train_step_multi: the consistency term / bounded linears need dist");
  CallLayout c;
  if (int rc = begin_call(plan, B, who, &c)) return rc;
  if (int rc = check_ws(plan, ws, c.save_slots, c.n_slabs, who)) return rc;
  inr::MlpArgs a = net_args(params, packed, coords, enc_B, B, c, ws);
  a.gt = gt;
  a.dist = dist;
  a.mask = mask;
  if (int rc = step_args(plan, ws, who, &a)) return rc;
  LossDesc ld;
  to_loss_desc(loss, &ld);
  return run_fused_step(plan, ld, a, c, grads, loss_out, params, packed, (hipStream_t)stream, who);
}

int inr_train_adam_step(const inr_plan* plan, const inr_loss_desc* loss, float* params, float* packed, const float* x,
                        const float* enc_B, const float* gt, const uint8_t* mask, int64_t B, const inr_workspace* ws,
                        float* grads, float* loss_out, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                        double beta2, double eps, double weight_decay, double l1, double l2, int32_t step,
                        void* stream) {
  if (grads == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr)
    return fail(INR_ERR_INVALID, "inr_train_adam_step: null argument");
  if (step < 1) return fail(INR_ERR_INVALID, "inr_train_adam_step: step %d (counts from 1)", step);
  if (plan != nullptr)
    if (int rc = check_real_penalty(plan, l1, l2, "inr_train_adam_step")) return rc;
  AdamFuse af;
  af.params = params, af.m1 = exp_avg, af.m2 = exp_avg_sq, af.packed = packed;
  af.aa = adam_args(beta1, beta2, eps, weight_decay, l1, l2);
  adam_bias_terms(lr, beta1, beta2, step, &af.aa.step_size, &af.aa.bc2_sqrt);
  return train_step_impl(plan, loss, params, packed, x, enc_B, gt, mask, B, ws, grads, loss_out, stream, &af);
}

#ifdef INR_STAMPS
// entries = 64 per WAVE of the grid (kernels index (blockIdx.x * waves_per_workgroup + wave) * 64 + stamp)
int inr_debug_set_stamp_buffer(long long* buf, long long entries) {
  g_stamp_buf = buf;
  g_stamp_cap = buf != nullptr ? entries : 0;
  return INR_OK;
}
#endif

}  // extern "C"
