// inr_host.h -- what the host files of the C-ABI share: inr_plan.hip (plan creation), inr_layout.hip (the launch layout of
// a call), inr_api.hip (the network entries), inr_api_offgrid.hip (the off-grid operators' entries) and inr_api_aux.hip
// (every other entry).  Host only: no kernel includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "../../include/inr_abi.h"
#include "inr_aux.h"
#include "inr_dw_gemm.h"
#include "inr_dw_gemm_bf16.h"

#pragma GCC visibility push(hidden)  // internal to the library: only the inr_* entries of inr_abi.h are exported

#ifdef INR_STAMPS
namespace inr {
extern long long* g_stamp_buf;  // diagnostic build only (make dbg): phase stamps of the fused kernels, entry / exit
extern long long g_stamp_cap;   // stamps of the GEMMs; entries behind it: a stamp whose index is not below this is dropped
}  // namespace inr
#endif

// the calling thread's error text (512 bytes, truncated; read back by inr_last_error): inr_plan.hip
int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
// how every entry ends once its launches are queued: the error in the entry's name, or INR_OK
inline int hip_done(hipError_t e, const char* what) { return e != hipSuccess ? hip_fail(e, what) : INR_OK; }
// a coil count `name` = v outside 1..INR_COIL_MAX; two byte ranges that share a byte (inr_api_aux.hip)
int coil_count_check(int32_t v, const char* name, const char* who);
bool ranges_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes);

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

constexpr int kMaxBlocks = 256;  // one persistent workgroup per CU (MI355X: 256 CUs)

struct inr_plan {
  inr_net_desc desc;
  NetDesc nd;
  int64_t packed_floats;
  // where a step's weight gradients come from, fixed at creation (plan_set_dw_route): 0 the fused kernels' own passes,
  // 1 the fp32 batch GEMM (inr_dw_gemm.hip), 2 the bf16 batch GEMM (inr_dw_gemm_bf16.hip).  Route 1: `gemm` holds what no
  // batch changes -- items, TL, WB, sizes; a call copies it and fills in tiles and chunks -- and `gemm_cover` the flat
  // range [lo, hi) or the layer mask those items cover
  int dw_route = 0;
  inr::DwGemmArgs gemm;
  inr::SlabSplit gemm_cover;
  // split steps (StepSchedule below): a low-priority stream for the part of the weight-gradient GEMM that runs beside
  // the fused kernel's last, partial round.  Created on first use, destroyed with the plan; the only state a plan has.
  mutable std::mutex side_mu;
  mutable hipStream_t side = nullptr;
  mutable int side_dev = -1;
  mutable hipEvent_t fork = nullptr, join = nullptr;  // the split step's two events, created with the side stream
  // bf16 plans: the gradient-scale state of the 8-bit stash (inr_w2.h), W2_STATE_FLOATS floats on the device, allocated
  // with the plan; what the host remembers about it: whether a kind of step (0 fused, 1 split) has been calibrated, and
  // for which batch size / loss.  One stream at a time may step a bf16 plan.
  mutable float* dz_state = nullptr;
  mutable int dz_dev = -1;
  mutable bool dz_ready[2] = {false, false};
  mutable int64_t dz_rows[2] = {0, 0};
  mutable int dz_loss[2] = {-1, -1};
  // Row-split plans keep two families of weight images in `packed`, one per fused kernel, and a step's update writes only
  // the family its own kernel reads (inr_train_adam_step under INR_LAZY_PACK=1; otherwise all of them).  img_valid = the IMG_* sets
  // (inr_aux.h) that hold the current parameters; an entry whose kernel reads a stale set re-packs it first, on its stream
  // (ensure_images, inr_api.hip).  Keyed to nothing: a plan serves ONE packed buffer between two inr_pack_params calls.
  // Every other plan has one family: always IMG_ALL.  img_eager: a call of this plan has been captured into a graph --
  // replays run no host code, so from then on every update writes every set (and a capturing call changes no state).
  mutable int img_valid = inr::IMG_ALL;
  mutable bool img_eager = false;
  // bf16 GEMM chunking knobs (tuning aids), read from the environment ONCE, when the plan is created: workspace sizes must
  // not depend on what the environment holds at the time of a later call
  bool gemm_one_class = false;
  double gemm_enc_cost = 0.0;  // 0: kEncCost
};

// gradient-scale state of a bf16 plan (inr_plan.hip)
float* dz_state_alloc(const inr_plan* p);
bool dz_needs_calibration(const inr_plan* p, int kind, int64_t rows, int loss_kind);
void dz_mark(const inr_plan* p, int kind, int64_t rows, int loss_kind);

// ---- the launch layout of a call (inr_layout.hip) ----
// split step: fused kernel on tiles [0, full), then on [full, nt) with `rem` workgroups; GEMM part A (tiles [0, tA)) on
// the side stream, part B behind the join
struct StepSchedule {
  bool split;
  int64_t full, rem, tA;
  inr::DwGemmArgs gA, gB;  // (split only)
  inr::SlabSplit red;      // for the reduction: n2 = all chunk slabs
};

// row-split fused step: `grid` workgroups run `rounds` tiles each; tile t has `hi` column blocks if t < x, else `lo`;
// `ncb` is the kernel build that runs them
struct RsSchedule {
  int grid, rounds, ncb, hi, lo, x;
};

// split row-split step (inr_layout.hip rs_split_schedule): `first` (256 tiles of `lo1` column blocks) and, behind its
// blk0 blocks, `rest` are the two launches; GEMM part A covers the first launch's slots [0, blk0 / 8), part B the others
struct RsSplit {
  bool split;
  int lo1, blk0;
  RsSchedule first, rest;
  inr::DwGemmArgs gA, gB;  // (split only)
  inr::SlabSplit red;      // for the reduction: n2 = all chunk slabs
};

// A function of the plan, the batch size and the two per-call environment switches, and of nothing else.  Every entry
// derives it ONCE (begin_call), checks the caller's workspace against it and launches from it, so the sizes that were
// checked are the sizes that are written.
struct CallLayout {
  int64_t nt, nb;               // tiles of the batch; workgroups of inr_mlp_kernel / the filter / bf16 kernels
  int64_t save_slots, n_slabs;  // a fused step's workspace: what inr_plan_workspace reports
  // dw_route 1
  bool rs;                      // the row-split kernel runs the fused step
  RsSchedule rsched;            // row-split plans (whichever kernel runs: the slabs cover its grid)
  RsSplit rsplit;               // how a step with gradients splits that launch; n_slabs covers it under every switch
  bool rs_split;                // this call may run it: rsplit.split, the row-split kernel chosen, INR_OVERLAP not 0
  inr::DwGemmArgs plain;        // the GEMM over the whole batch: unfused backward, row-split and unsplit steps
  inr::SlabSplit plain_red;
  StepSchedule step;            // (split = false on every other route)
  // dw_route 2
  inr::DwGemmBf16Args bf16;
  inr::SlabSplit bf16_red;
};

// B >= 1.  INR_RS and INR_OVERLAP are read here, per call: tests flip them between calls on one plan in one process
void call_layout(const inr_plan* plan, int64_t B, CallLayout* c);
// B and, from it, the call's layout: the one place an entry learns its tiles, grids, chunks and workspace
int begin_call(const inr_plan* plan, int64_t B, const char* who, CallLayout* c);

// ---- validity of the weight-image sets (inr_layout.hip: pure; inr_plan.hip: the plan's state) ----
enum { IMG_EV_PACK = 0, IMG_EV_UPDATE = 1, IMG_EV_READ = 2 };  // what happened to the sets named with it
enum { IMG_CALL_FORWARD = 0, IMG_CALL_BACKWARD = 1, IMG_CALL_STEP = 2 };
// the valid sets after `event`: a pack or a read (= re-pack of what was stale) adds `sets`, an update leaves `sets` alone valid
int image_sets_after(int valid, int event, int sets);
// the sets a network call of a row-split plan reads: its fused step those of the kernel that runs it (`row_split`),
// forward and backward inr_mlp_kernel's
int image_sets_read(int call, bool row_split);
// INR_LAZY_PACK=1 in the environment (read per call, like INR_RS)
bool lazy_pack_enabled();
// is `st` capturing a graph?  (errors count as no)
bool stream_capturing(hipStream_t st);
// the sets an update of this call may leave out, given the sets its step reads; 0 where the plan, the switch or a capture
// says eager
int image_sets_skip(const inr_plan* plan, int reads, hipStream_t st);
// after a launch that wrote (`event` PACK / READ) or left only (`event` UPDATE) `sets`: the plan's new state
void images_note(const inr_plan* plan, int event, int sets, hipStream_t st);

// ---- shared by inr_api.hip and inr_api_aux.hip (defined in the latter) ----
void to_loss_desc(const inr_loss_desc* l, LossDesc* o);
int check_real_penalty(const inr_plan* plan, double l1, double l2, const char* who);
void adam_bias_terms(double lr, double beta1, double beta2, int32_t step, float* step_size, float* bc2_sqrt);
inr::AdamArgs adam_args(double beta1, double beta2, double eps, double weight_decay, double l1, double l2);

#pragma GCC visibility pop
