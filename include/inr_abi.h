/*
 * inr_abi.h -- C-ABI of libinr_mi355x.so, the MI355X (gfx950) engine for the coordinate-MLP
 * fitting hot path of luisdavid64/MRI-Implicit-Neural-Representations.
 *
 * The reference has no FFI: the path sits behind torch.nn.Module + torch.optim.
 * Each entry point below names the reference code it replaces (paths under /root/reference/src).
 * Conventions:
 *   - every function returns 0 on success, <0 on error; inr_last_error() gives the message
 *     (thread-local); nothing throws or aborts across the ABI;
 *   - all tensor arguments are DEVICE pointers to contiguous row-major fp32 buffers owned by the
 *     caller -- except inr_image_metrics' `metrics_out` and `scratch`, which are fp64 (double) device buffers, and
 *     inr_shuffle_epoch's integer buffers (uint8 masks, int32 counts, int64 order), inr_gray8's uint8 `lut` / `out` and
 *     inr_coil_stats' and inr_band_stats' fp64 `stats` / `scratch` (inr_band_stats' bounds are host arrays) and
 *     inr_coil_gram's fp64 `gram` / `scratch`; the
 *     library retains no pointer across calls and allocates no device memory -- with ONE exception:
 *     an INR_PRECISION_BF16 plan owns 64 bytes of device memory (16 words), its gradient-scale state (inr_plan_grad_scale_state),
 *     allocated with hipMalloc and initialised with a synchronous hipMemcpy by the first call that needs it on a device
 *     (a step, a backward, or inr_plan_grad_scale_state), freed by inr_plan_destroy.  That first call must therefore run
 *     OUTSIDE stream capture;
 *   - all work is ordered on the hipStream_t passed as `stream` (void*); no implicit sync.  One exception to
 *     "enqueued on": a fused step whose tiles leave the last round of the persistent grid partly empty runs part of
 *     its weight-gradient GEMM on a low-priority side stream the plan creates on first use, forked from and joined
 *     back into `stream` with events inside the call (csrc/inr_layout.hip step_schedule; INR_OVERLAP=0 disables it) --
 *     to the caller the call still behaves as work on `stream`, including under stream capture;
 *   - a plan's description is immutable after creation (that side stream, and a bf16 plan's scale state, are its only state) and it may be shared
 *     between threads and streams as long as each in-flight call has its own workspace buffers.
 *
 * Parameter layout ("flat params", P floats): layer k's weight [M_k, K_k] (PyTorch [out,in]
 * layout) followed by its bias [M_k], k = 0..D-1 -- i.e. the reference's state_dict order
 * (SIREN: model.{k}.linear.weight/bias, networks.py:79,114-117; FFN: model.{2k}.weight/bias,
 * networks.py:57-62; WIRE: net.{k}.linear.weight/bias + net.{depth+1}.weight/bias with complex64
 * tensors stored as interleaved (re, im) float pairs = torch.view_as_real; the frozen
 * omega_0/scale_0 Parameters are NOT part of the flat buffer).  Gradients (torch's convention
 * dL/dRe + j dL/dIm for complex tensors) and Adam moments use the same layout.
 */
#ifndef INR_ABI_H
#define INR_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7: inr_adam_step_shard (data-parallel update on the entries a rank owns), inr_reg_grad (penalty gradients, complex64 tensors
 *    included; the Adam entry points refuse l1 / l2 != 0 on plans with complex tensors).
 *    v7 additions (no version change: nothing existing moved): inr_image_metrics_scratch, inr_image_metrics (RSS, PSNR, SSIM of
 *    the validation epoch); inr_shuffle_epoch (the keyed row permutation of a shuffled epoch); inr_kspace_display, inr_gray8,
 *    inr_coil_stats and their scratch queries (the pictures and the per-coil table of the validation epoch); inr_grid_rows
 *    (rows of a coordinate grid, made on the device: reconstruction from a checkpoint on any grid); inr_band_stats and its
 *    scratch query (per-band counts, energies, errors and extrema of a field against radius); inr_coil_gram, its scratch
 *    query and inr_coil_apply (software coil compression: the coil Gram matrix in one pass, the product with a small matrix);
 *    inr_nudft and its scratch query (the continuous k-space of coil images at off-grid positions); inr_adjoint_nudft and
 *    its scratch query (its conjugate transpose: off-grid samples back onto the image grid); inr_plan_image_sets,
 *    inr_image_sets_after and inr_image_sets_read (weight images on demand: see inr_pack_params); inr_nufft_prepare,
 *    inr_nufft_interp, inr_nufft_spread, inr_nufft_finish and their scratch query (the same two operators by
 *    Kaiser-Bessel gridding around the caller's FFT); inr_ring_scale (rows divided by the divisor of the ring their radius
 *    lies in: ring-normalised fits); inr_row_cdf, its scratch query and inr_sample_epoch (weighted epochs: an integer
 *    CDF of per-row weights and a stratified draw of an epoch's rows from it); inr_plan_step_split (how a row-split
 *    step with gradients is split over two launches and two GEMM parts); inr_radial_scale (rows divided or multiplied
 *    by a piecewise-linear radial profile: ring normalisation without jumps at the ring edges); inr_gain_loss_grad and
 *    inr_gain_apply (a learned radial gain: the backbone's output times exp(-s) of a second network, the loss on the
 *    product and its gradients to both in one pass); inr_focal_loss_grad (the focal frequency loss: rows weighted by
 *    their own error relative to the batch's largest, in two passes); inr_mix_loss_grad and inr_mix_apply (a mixture of
 *    heads: K experts' outputs mixed by a gate network's weights, the loss on the mix plus each expert's own loss on its
 *    k-space ring, and the gradients to all of them in one pass); inr_sense_apply and inr_sense_grad (SENSE-model fits:
 *    coil images as the product of an image network and a sensitivity network in image space, written where ifftshift
 *    puts them, and the adjoint of that product); inr_sense_lowres, inr_sense_maps and inr_sense_adjoint (SENSE fits on
 *    coil maps calibrated from the centre of k-space: low-resolution coil images of the centre block on any grid, their
 *    unit-RSS maps, and the image half of inr_sense_grad alone); inr_image_tv_grad (a total-variation prior on the
 *    image of a SENSE fit: smoothed isotropic TV of the image network's output, its value and its gradient in one gather
 *    pass); inr_sense_nufft_prepare, inr_sense_nufft_finish, inr_nufft_interp_plain and inr_nufft_spread_plain (off-grid
 *    SENSE fits: the coil product fused with the gridding operators on a grid laid out as a plain FFT reads it).
 * 6: inr_plan_step_info, inr_loss_tv_grad, 16-word gradient-scale state.  5: bf16 plans.  4: inr_adam_step_dev.  3: inr_workspace. */
#define INR_ABI_VERSION 7

/* error codes */
#define INR_OK 0
#define INR_ERR_INVALID (-1)     /* bad argument (null pointer, B <= 0, unsupported shape) */
#define INR_ERR_UNSUPPORTED (-2) /* valid request the engine has no kernel for */
#define INR_ERR_HIP (-3)         /* a HIP runtime call failed */

/* network family: which reference class the plan mirrors */
enum inr_kind {
  INR_KIND_SIREN = 0, /* models/networks.py:99-124  SIREN / SirenLayer :74-96 */
  INR_KIND_FFN = 1,   /* models/networks.py:48-69   FFN (ReLU hidden, Sigmoid output) */
  INR_KIND_WIRE = 2,  /* models/networks.py:206-260 WIRE / ComplexGaborLayer :160-204 (complex64 layers) */
  INR_KIND_FOURIER = 3,   /* models/mfn.py:61-94    FourierNet (one output_linear after the last stage) */
  INR_KIND_MSFOURIER = 4, /* models/mfn.py:206-267  MultiscaleKFourier: heads output_linear[i], i in [1,3,5,7];
                             the unused last stage / heads exist in flat params but are never evaluated or
                             stepped (the reference leaves their .grad = None) */
  INR_KIND_MSBOUNDED = 5, /* models/mfn.py:288-355  MultiscaleBoundedFourier: BoundedLinear (:269-286) zeroes the rows
                             of h whose dist lies outside [lo,hi] before each hidden Linear */
  INR_KIND_GABOR = 6,     /* models/mfn.py:133-162  GaborNet: GaborLayer filters (:96-131)
                             sin(F x + c) * exp(-0.5 * gamma_j * |x - mu_j|^2), mu and gamma trainable */
  INR_KIND_KGABOR = 7,    /* models/mfn.py:164-204  KGaborNet: same arithmetic (dist_to_center is passed to the
                             filters but with_dist_filtering is never enabled); the dist argument is ignored */
  INR_KIND_WIRE2D = 8     /* models/wire2d.py:62-117 WIRE2D / ComplexGaborLayer2D :3-60: two Linears per layer
                             (linear, scale_orth), width NOT reduced; flat params interleave them per layer.
                             inr_forward needs a save buffer (the orth terms travel through it). */
};

/* arithmetic of the three GEMM loops (accumulation, master weights and Adam are fp32 in both) */
enum inr_precision {
  INR_PRECISION_F32 = 0,  /* v_mfma_f32_32x32x2_f32: the parity path (1e-5 against the reference's fp32) */
  INR_PRECISION_BF16 = 1  /* v_mfma_f32_32x32x16_bf16 on bf16-rounded operands + hardware sin/cos: throughput path
                             for SIREN + fused gauss encoder, width 129..256; always needs the save buffer */
};

/* activation of the last layer */
enum inr_act {
  INR_ACT_ID = 0,      /* network_last_linear: True (default), networks.py:96 */
  INR_ACT_SIN = 1,     /* sin(w0 z): hidden SIREN layers; last layer if network_last_linear False */
  INR_ACT_TANH = 2,    /* last_tanh: True, networks.py:94-95 */
  INR_ACT_RELU = 3,    /* FFN hidden, networks.py:57-60 */
  INR_ACT_SIGMOID = 4, /* FFN output, networks.py:63 */
  INR_ACT_CTANH = 7    /* WIRE2D last_tanh: torch.nn.Tanh() on the complex output before .real (wire2d.py:106-107,
                          113-117); out_features <= 2 */
};

/* how the first layer's input is produced */
enum inr_input {
  INR_INPUT_X = 0,     /* x [B, in_features] already in memory (what model.forward receives,
                          train.py:163-169: coords = encoder.embedding(coords); model(coords)); every kind,
                          the filter networks of models/mfn.py included (mfn.py:34-43,85-94,255-267) */
  INR_INPUT_GAUSS = 1  /* fused Positional_Encoder 'gauss' (networks.py:30-33): coords [B,3] and
                          enc_B [E,3]; in_features must equal 2E; [B,2E] is never materialised */
};

/* pointwise losses the fused train step can evaluate in-kernel (others: inr_loss_grad + tier 1) */
enum inr_loss {
  INR_LOSS_L2_HALF = 0, /* 0.5 * torch.nn.MSELoss()   train.py:82,182 */
  INR_LOSS_L1_HALF = 1, /* 0.5 * torch.nn.L1Loss()    train.py:92,182 */
  INR_LOSS_TANH = 2,    /* TanhL2Loss                 metrics/losses.py:130-139 */
  INR_LOSS_LOGSPACE = 3,/* LogSpaceLoss               metrics/losses.py:214-223 */
  INR_LOSS_HDR = 4,     /* HDRLoss_FF (separable form) metrics/losses.py:236-264 */
  INR_LOSS_MSLE_HALF = 5, /* 0.5 * MSLELoss()          metrics/losses.py:18-27; train.py:84,182 */
  INR_LOSS_CENTER = 6    /* CenterLoss ('LSL' of train.py:87-88), pointwise part: metrics/losses.py:141-173,201;
                            its random-pair term is inr_center_pairs_grad */
};

typedef struct inr_net_desc {
  int32_t kind;         /* enum inr_kind */
  int32_t in_features;  /* net.network_input_size */
  int32_t width;        /* hidden features: net.network_width for SIREN / FFN / MFN / WIRE2D (1..512; WIRE2D counts
                           complex features, <= 256); for WIRE the number of COMPLEX hidden features,
                           int(network_width / sqrt(2)) (networks.py:228), <= 192.  Widths between the built
                           block counts run zero-padded. */
  int32_t depth;        /* net.network_depth as the reference counts it: all Linear layers for SIREN/FFN,
                           hidden complex layers only for WIRE (total Linear = depth + 2) */
  int32_t out_features; /* net.network_output_size, 1..4 */
  int32_t last_act;     /* enum inr_act */
  int32_t input;        /* enum inr_input */
  int32_t enc_size;     /* E (encoder.embedding_size) when input == INR_INPUT_GAUSS */
  float w0;             /* 30 for SIREN (networks.py:75); ignored otherwise */
  float first_omega_0;  /* WIRE net.first_omega_0 */
  float hidden_omega_0; /* WIRE net.hidden_omega_0 */
  float scale_0;        /* WIRE net.scale */
  int32_t precision;   /* enum inr_precision; 0 (the default of a zeroed struct) = exact fp32 */
  int32_t reserved[3];
} inr_net_desc;

typedef struct inr_loss_desc {
  int32_t kind;       /* enum inr_loss */
  float eps;          /* loss_opts.hdr_eps */
  float sigma;        /* loss_opts.hdr_ff_sigma */
  float factor;       /* loss_opts.hdr_ff_factor */
  float inv_count;    /* 1 / (number of rows entering the mean, summed over all ranks) */
  float hdr_A;        /* mean_i((1-f_i)^2) over the batch's kcoords (HDR only) */
  float scale;        /* multiplies the pointwise loss; 0 means 1.  The multiscale loop uses 0.5*loss_fn
                         (train_kspace_multiscale.py:188-190): 0.5 for LogSpace, 1 for the *_HALF kinds */
  /* ConsistencyLoss between consecutive heads (metrics/losses.py:315-324; multiscale kinds only) */
  float cons_w;       /* 0.1 (train_kspace_multiscale.py:179); 0 disables */
  int32_t cons_chan;  /* 2: dist is [B] (rows compared); 1: per-coil dist [B,1] -> channel 0 only */
  float cons_lo[4], cons_hi[4]; /* bounds[i] of pair i: rows with dist < lo or dist > hi are compared */
  float cons_inv[4];  /* 1 / (number of compared elements of pair i over all ranks); 0 when the pair is empty */
} inr_loss_desc;

typedef struct inr_plan inr_plan;

/* Caller-owned scratch of one call, with its extents so that a short buffer is INR_ERR_INVALID and never an
 * out-of-bounds GPU write.  `save` = the activation stash (slots of inr_sizes.save_bytes_per_tile), `slabs` = the
 * gradient slabs (of inr_sizes.slab_floats floats); how many of each a batch of B rows needs:
 * inr_plan_launch_dims / inr_plan_workspace.  Extents are in floats. */
typedef struct inr_workspace {
  float* save;
  int64_t save_floats;
  float* slabs;
  int64_t slab_floats;
} inr_workspace;

/* sizes (in bytes unless stated) a caller needs to allocate buffers for a plan */
typedef struct inr_sizes {
  int64_t n_params;        /* P: floats in flat params / grads / Adam moments */
  int64_t packed_floats;   /* floats in the MFMA-fragment-ordered weight image */
  int64_t tile_rows;       /* coordinates per workgroup tile (128) */
  int64_t save_bytes_per_tile; /* activation stash per tile (tier 1: n_tiles of them) */
  int64_t max_blocks;      /* upper bound on the persistent grid (slab count) */
  int64_t slab_floats;     /* floats per gradient slab (= P + 4 loss words, padded) */
  int64_t step_save_by_tile; /* inr_train_step_multi's `save`: 1 = n_tiles slots, 0 = n_blocks slots */
} inr_sizes;

int inr_abi_version(void);
/* copies the calling thread's last error message; returns its length */
int inr_last_error(char* buf, size_t cap);

/* Replaces: SIREN.__init__ / FFN.__init__ shape bookkeeping (networks.py:100-119, 49-65). */
int inr_plan_create(const inr_net_desc* desc, inr_plan** out);
int inr_plan_destroy(inr_plan* plan);
int inr_plan_sizes(const inr_plan* plan, inr_sizes* out);
/* number of tiles / persistent blocks / workspace bytes for a batch of B rows */
int inr_plan_launch_dims(const inr_plan* plan, int64_t B, int64_t* n_tiles, int64_t* n_blocks);
/* buffers of a training step on B rows: `save` slots (of save_bytes_per_tile) that inr_train_step /
 * inr_train_step_multi need -- n_tiles for plans whose weight gradients come from the batch-level GEMM
 * (inr_sizes.step_save_by_tile), n_blocks otherwise -- and the number of slabs (of slab_floats) behind `slabs` for
 * the step and backward entry points: n_blocks, plus one per K-chunk of that GEMM. */
int inr_plan_workspace(const inr_plan* plan, int64_t B, int64_t* step_save_slots, int64_t* n_slabs);
/* (v6) Which kernel runs the fused step (inr_train_step*) of a batch of B rows, for benchmarks and tests; no reference
 * counterpart.  row_split = 1: inr_mlp_rs_kernel<ncb, .> -- the four waves of a workgroup split the OUTPUT rows of every layer
 * and share the tile's coordinates, dealt in column blocks of 16 (SIREN / FFN behind the fused gauss encoder, hidden width
 * 129..256): `grid` workgroups run `rounds` tiles each, tile t = round * grid + workgroup holds `hi` blocks if t < n_hi, else
 * `lo`.  row_split = 0: the plan's per-coordinate-tile kernel (inr_mlp_kernel, inr_mfn_kernel, inr_siren_bf16_kernel, ...):
 * grid = n_blocks of inr_plan_launch_dims, rounds = ceil(n_tiles / grid), the other fields 0. */
typedef struct inr_step_info {
  int32_t row_split, ncb, grid, rounds, hi, lo, n_hi;
  int32_t hidden_blocks; /* 32-row blocks of the hidden images in the plan's kernel build (either kernel; was reserved = 0) */
} inr_step_info;
int inr_plan_step_info(const inr_plan* plan, int64_t B, inr_step_info* out);
/* (v7) How a row-split step WITH gradients is launched, for tests and tools; no reference counterpart.  inr_plan_step_info
 * goes on describing the single launch (what a call without gradients, a capturing call and INR_OVERLAP=0 run).  Where
 * that launch is one round of 256 workgroups with a few tiles one column block wider than the rest, the step is split:
 * a first launch of 256 tiles of `lo1` blocks, then -- beside part A of the weight-gradient GEMM, which needs the first
 * launch's stash slots only -- a remainder launch of the other blocks, and behind it part B of the GEMM over the
 * remainder's slots.  out[0] engaged (0: out[1..14] are 0) -- the layout a call MAY run: without its second stream (creation
 * failed) a step keeps the single launch, with the same results; [1] lo1; the remainder launch: [2] hi, [3] lo, [4] n_hi
 * (as in inr_step_info, its blocks behind the first 256 lo1), [5] workgroups, [6] ncb; part A: [7] slots [0, out[7]),
 * [8] slots per chunk, [9] chunks, [10] workgroups; part B: [11] first slot (slots up to n_tiles), [12] slots per
 * chunk, [13] chunks, [14] workgroups; [15] n_slabs of inr_plan_workspace. */
#define INR_STEP_SPLIT_WORDS 16
int inr_plan_step_split(const inr_plan* plan, int64_t B, int64_t* out);
/* INR_PRECISION_BF16 plans (v5; 16 words since v6).  Their backward pass stashes dZ in 8 bits under a power-of-two scale that
 * follows the gradient's magnitude from step to step; the sixteen words of that state live on the device with the plan (layout:
 * csrc/inr_w2.h -- [0..3] fused steps, [4..7] split steps: next scale, bits of the last step's largest scaled |dZ|, the
 * factor the last step multiplied d(loss)/d(out) by, the scale inside it; [8], [9] fused steps so far whose gradients were
 * clipped at bf8's largest finite value / mostly flushed under its subnormals, [10], [11] the same for split steps -- the scale
 * lags the gradient by one step and has 2^10.8 of headroom; [12..15] zero).  This call waits for the work queued on
 * `stream` and copies them to host_out[16]: for tests and diagnostics (no reference counterpart).  Because of this state a
 * bf16 plan is to be stepped from one stream at a time; the plan's first step of a kind, and a step whose loss or batch
 * size makes the remembered scale meaningless, runs the kernel twice (once to find the scale). */
int inr_plan_grad_scale_state(const inr_plan* plan, float* host_out, void* stream);

/* Re-orders flat params into the MFMA A-fragment image the kernels stream (no reference
 * counterpart: it is what `model.to(device)` + ATen's GEMM packing do implicitly). */
int inr_pack_params(const inr_plan* plan, const float* params, float* packed, void* stream);

/* Weight images on demand (no reference counterpart).  Plans whose fused step has two kernels to choose from per batch
 * (inr_plan_step_info: row_split) keep one family of weight images in `packed` for each: the forward (INR_IMG_FWD) and
 * transposed (INR_IMG_TR) images of the kernel behind inr_forward / inr_backward and behind steps with row_split == 0,
 * and the fragment images (INR_IMG_RS) of the row-split kernel.  With INR_LAZY_PACK=1 in the environment (read per call;
 * unset or 0: every update writes every set) inr_train_adam_step rewrites only the family its own step read and the plan
 * remembers the others as stale; any later inr_forward, inr_backward, inr_train_step or
 * inr_train_adam_step whose kernel reads a stale set first re-packs it from `params`, on its own stream -- so these
 * entries may WRITE to their `packed` argument, with exactly what inr_pack_params would have put there.  Bias tables
 * are written by every update.  inr_pack_params, inr_adam_step and inr_adam_step_dev write every set.
 * The state lives in the plan and is keyed to nothing else: between two inr_pack_params calls a plan serves ONE packed
 * buffer (and one params vector); hand a plan another buffer only through inr_pack_params.  Like a bf16 plan's scale
 * state it wants the plan stepped from one stream at a time.
 * A call made while its stream
 * is capturing a graph changes no state, re-packs what it finds stale inside the graph, and ends the plan's laziness
 * for good: a replay runs no host code that could notice a stale set.
 * inr_plan_image_sets: the sets that hold the current parameters, and whether the next update may leave some out.
 * inr_image_sets_after / inr_image_sets_read: the rules themselves, as pure functions (tests): the valid sets after
 * `event` happened to `sets`; the sets a call reads. */
#define INR_IMG_FWD 1
#define INR_IMG_TR 2
#define INR_IMG_RS 4
#define INR_IMG_EV_PACK 0   /* `sets` were written from the current parameters */
#define INR_IMG_EV_UPDATE 1 /* the parameters moved and only `sets` were rewritten */
#define INR_IMG_EV_READ 2   /* a call that reads `sets` re-packed the stale ones among them */
#define INR_IMG_CALL_FORWARD 0
#define INR_IMG_CALL_BACKWARD 1
#define INR_IMG_CALL_STEP 2
int inr_plan_image_sets(const inr_plan* plan, int32_t* valid, int32_t* lazy);
int inr_image_sets_after(int32_t valid, int32_t event, int32_t sets);
int inr_image_sets_read(int32_t call, int32_t row_split);

/* Replaces Positional_Encoder.embedding, 'gauss' (networks.py:30-33): out [B, 2E]. */
int inr_encode_gauss(const float* coords, const float* enc_B, int64_t B, int32_t E, float* out,
                     void* stream);

/* Replaces Positional_Encoder.embedding, 'LogF' (networks.py:16,24-29): bands [n_bands] =
 * 2^linspace(0, scale, n_bands); out [B, 6*n_bands] = per axis [sin(2 pi x_a b) | cos(2 pi x_a b)]. */
int inr_encode_logf(const float* coords, const float* bands, int64_t B, int32_t n_bands, float* out,
                    void* stream);

/* Replaces model.forward (networks.py:121-124 / 67-69).  `x` is [B,in_features] (INR_INPUT_X) or
 * coords [B,3] (INR_INPUT_GAUSS, with enc_B [E,3]).  out [B,out_features].  `ws` may be NULL (or ws->save NULL)
 * for a no_grad forward (train.py:203-220); otherwise ws->save receives n_tiles stash slots. */
int inr_forward(const inr_plan* plan, const float* params, const float* packed, const float* x,
                const float* enc_B, int64_t B, float* out, const inr_workspace* ws, void* stream);

/* Replaces loss.backward() through the model (train.py:189): given d(loss)/d(out) [B,out_features]
 * and the forward's stash (ws->save, n_tiles slots), writes d(loss)/d(params) into grads [P].  ws->slabs holds
 * n_slabs slabs (inr_plan_workspace).  The stash is CONSUMED: plans with inr_sizes.step_save_by_tile overwrite
 * act'(z_l) with dZ_l, the operand of their weight-gradient GEMM. */
int inr_backward(const inr_plan* plan, const float* params, const float* packed, const float* x,
                 const float* enc_B, int64_t B, const float* dout, const inr_workspace* ws,
                 float* grads, void* stream);

/* Replaces the loss modules + their autograd (train.py:178-182; metrics/losses.py): writes
 * dout [B,2] = d(loss)/d(out) and accumulates the scalar loss into loss_out[0] (device).
 * `mask` (may be NULL) is one byte per row: rows with 0 do not enter the loss (train.py:172-177).
 * `kcoords` is never read and may be NULL (the HDR weight's batch mean travels in loss->hdr_A); the argument stays
 * for the ABI's sake. */
int inr_loss_grad(const inr_loss_desc* loss, const float* out, const float* gt, const float* kcoords,
                  const uint8_t* mask, int64_t B, float* loss_out, float* dout, void* stream);

/* Multi-head form for the multiscale loop (train_kspace_multiscale.py:176-195): outs / douts are [n_heads][B][2]
 * (what inr_forward_multi writes / inr_backward_multi reads); the pointwise terms (scale * loss_fn, summed over
 * heads) see the rows with mask != 0, ConsistencyLoss (cons_* fields, metrics/losses.py:315-324) every row. */
int inr_loss_grad_multi(const inr_loss_desc* loss, const float* outs, const float* gt, const float* dist,
                        const uint8_t* mask, int32_t n_heads, int64_t B, float* loss_out, float* douts, void* stream);

/* Replaces tv_loss (metrics/losses.py:326-343) + its autograd on one coil's predicted k-space
 * (train.py:173-175, train_kspace_multiscale.py:173-175; per-coil batches from
 * MRICoilWrapperDataset, data/nerp_datasets.py:397-441):
 *   weight * ( mean|img[:, :-1] - img[:, 1:]| + mean|img[:-1] - img[1:]| ),  img [H][W][2].
 * `out` [R][W][2] holds R consecutive image rows of which the first R_own belong to the caller;
 * a data-parallel rank passes its rows plus one halo row (R = R_own + 1) so that every vertical
 * pair is counted by exactly one rank, and the single-GPU call passes R = R_own = H.  The means
 * are over the whole image (H), so per-rank losses and gradients sum to the reference's.
 * ADDS the gradient into dout [R][W][2] and the loss into loss_out[0]; loss_out[1..64] is scratch
 * (same layout as inr_loss_grad, which is normally called first on the same buffers). */
int inr_tv_grad(const float* out, int64_t R, int64_t R_own, int64_t W, int64_t H, float weight,
                float* loss_out, float* dout, void* stream);

/* (v6) inr_loss_grad + inr_tv_grad of one coil's rows in one pass -- the per-coil step of train.py:163-189 with use_tv:
 * the masked pointwise loss (train.py:176-182) on the rows the caller owns (r < R_own; a data-parallel rank's halo row stays
 * with its owner: no zeroed copy of the mask is needed) plus tv_loss (metrics/losses.py:326-343, arguments as inr_tv_grad).
 * out / gt / dout [R][W][2], mask [R][W] bytes or NULL.  WRITES dout (does not add) and loss_out[0] = pointwise + TV loss;
 * loss_out[1..256] is scratch: a loss_out buffer holds INR_LOSS_WORDS floats. */
#define INR_LOSS_WORDS 512
int inr_loss_tv_grad(const inr_loss_desc* loss, const float* out, const float* gt, const uint8_t* mask, int64_t R,
                     int64_t R_own, int64_t W, int64_t H, float tv_weight, float* loss_out, float* dout, void* stream);

/* Replaces the random-pair ("centre") term of CenterLoss.forward (metrics/losses.py:175-199; 'LSL' of train.py:87-88,
 * called at train.py:178-180) for ONE radial band: the caller draws the n row pairs (idx_a[p] from the inner mask, idx_b[p]
 * from the ring outside it) with torch.randperm exactly as the reference does (losses.py:193-194) and passes global row
 * indices into out / gt [B,2];  r_p = (|gt_a| - |gt_b|) - (|out_a| - |out_b|).  ADDS  weight * mean_p r_p^2  to loss_out[0]
 * (loss_out[1..64] is scratch, same layout as inr_loss_grad) and its gradient to dout [B,2].  Call after inr_loss_grad with
 * INR_LOSS_CENTER on the same buffers (weight = 0.1 per band, losses.py:201), before inr_backward. */
int inr_center_pairs_grad(const float* out, const float* gt, const int64_t* idx_a, const int64_t* idx_b, int64_t n,
                          int64_t B, float weight, float* loss_out, float* dout, void* stream);

/* Fused tier-2 step, stages 1-3 of train.py:163-189 in one launch: encode -> forward -> pointwise
 * loss -> backward, then the fixed-order slab reduction.  Leaves grads [P] and loss_out[0];
 * the caller all-reduces grads across ranks (if any) and calls inr_adam_step.  `grads` may be
 * NULL to launch the fused kernel alone and leave the slabs unreduced (used to time it).
 * The complex-row losses (INR_LOSS_LOGSPACE and above: they read an output row as one complex number) need
 * out_features == 2; every fused entry point -- this one, inr_train_adam_step, inr_train_step_multi -- refuses them
 * on any other plan with INR_ERR_INVALID. */
int inr_train_step(const inr_plan* plan, const inr_loss_desc* loss, const float* params,
                   const float* packed, const float* x, const float* enc_B, const float* gt,
                   const uint8_t* mask, int64_t B, const inr_workspace* ws, float* grads,
                   float* loss_out, void* stream);

/* Multi-head networks (MultiscaleKFourier.forward returns a list, mfn.py:255-267): `out` / `dout` are
 * [n_heads][B][out_features]; `coords` is coords [B,3] with enc_B [E,3] (INR_INPUT_GAUSS plans) or the encoded
 * x [B,in_features] with enc_B NULL (INR_INPUT_X plans: what the reference's forward receives, mfn.py:34-43);
 * `dist` [B] = dist_to_center (nerp_datasets.py:385), read by the consistency term and the bounded linears;
 * ws->save is always required (it also carries the input features between stages;
 * pass n_blocks slots and by_block = 1 for a no_grad sweep, n_tiles slots and 0 before inr_backward_multi).
 * inr_backward_multi CONSUMES the stash: plans with inr_sizes.step_save_by_tile overwrite stashed factors with
 * the gradient operands of their batch-level weight-gradient GEMM, so one forward serves one backward.
 * inr_train_step_multi takes n_tiles slots when step_save_by_tile is set, n_blocks slots otherwise. */
int inr_forward_multi(const inr_plan* plan, const float* params, const float* packed, const float* coords,
                      const float* enc_B, const float* dist, int64_t B, float* out, const inr_workspace* ws,
                      int32_t by_block, void* stream);
int inr_backward_multi(const inr_plan* plan, const float* params, const float* packed, const float* coords,
                       const float* enc_B, const float* dist, int64_t B, const float* dout,
                       const inr_workspace* ws, float* grads, void* stream);
/* MultiscaleBoundedFourier(boundaries=pairs_model) (train_kspace_multiscale.py:85,95): one (lo,hi) per hidden
 * Linear; must be called before the plan is used (dist may be NULL for the other kinds above). */
int inr_plan_set_bounds(inr_plan* plan, const float* lo, const float* hi, int32_t n);
int inr_train_step_multi(const inr_plan* plan, const inr_loss_desc* loss, const float* params,
                         const float* packed, const float* coords, const float* enc_B, const float* gt,
                         const float* dist, const uint8_t* mask, int64_t B, const inr_workspace* ws,
                         float* grads, float* loss_out, void* stream);
int inr_plan_heads(const inr_plan* plan, int32_t* n_heads);

/* Replaces torch.optim.Adam.step (train.py:76,190; eps 1e-8, amsgrad False, L2-style
 * weight_decay) plus the L1/L2 "regularization" gradient terms (models/regularization.py:21-36),
 * and refreshes `packed` for the next forward.  `step` counts from 1.  Hyper-parameters are
 * doubles because torch derives step_size = lr / (1 - beta1^t) etc. in Python doubles. */
int inr_adam_step(const inr_plan* plan, float* params, const float* grads, float* exp_avg,
                  float* exp_avg_sq, float* packed, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double l1, double l2, int32_t step, void* stream);

/* Replaces the backward of `train_loss += regularization(model.parameters())` (train.py:185-187;
 * models/regularization.py:21-36) for ANY plan, complex64 tensors included (WIRE / WIRE2D: interleaved (re, im) pairs in
 * the flat vector): adds to grads[i - lo], lo <= i < hi, the gradient of
 *   l1 * sum |p|         -- real entries sign(p); a complex entry z contributes |z|: (re, im) / |z|, 0 at z = 0
 *   l2 * |S|, S = sum p^2 over every Parameter -- complex when the model has complex tensors (z^2 = a^2 - b^2 + 2iab):
 *                           with u = conj(S) / |S|: real entry 2 p Re(u); d/d re = 2 Re(u z), d/d im = -2 Im(u z).
 * `l2_dir` = device pointer to (Re u, Im u); NULL means (1, 0) and is required to be non-NULL only for l2 != 0 on a plan
 * with complex tensors.  The caller forms S -- it also holds the squares of the frozen omega_0 / scale_0 Parameters
 * (networks.py:191-192), which the flat vector does not carry -- and the penalty VALUE it logs.  The Adam entry points
 * form the real-entry terms themselves (l1, l2 arguments) and refuse l1 / l2 != 0 on plans with complex tensors: there,
 * call this first and pass them 0.  [lo, hi) = [0, P) for a whole gradient, or a rank's chunk before inr_adam_step_shard. */
int inr_reg_grad(const inr_plan* plan, const float* params, float* grads, int64_t lo, int64_t hi, double l1,
                 double l2, const float* l2_dir, void* stream);

/* The update of a data-parallel job whose ranks each own 1/N of the flat parameter vector (no reference counterpart:
 * train_kspace_multiscale.py:161-201 is single-process; this is torch.optim.Adam on a slice): the same arithmetic as
 * inr_adam_step on the entries [lo, hi) only.  `grads_shard[i - lo]` is the summed gradient of entry i -- the rank's
 * chunk of a reduce-scatter of the flat gradient; params / exp_avg / exp_avg_sq are the full-length vectors (only
 * [lo, hi) is read and written).  No image is refreshed: after the all-gather of the updated parameters every rank calls
 * inr_pack_params.  lo == hi is a no-op (a rank whose chunk lies in the padding). */
int inr_adam_step_shard(const inr_plan* plan, float* params, const float* grads_shard, float* exp_avg,
                        float* exp_avg_sq, int64_t lo, int64_t hi, double lr, double beta1, double beta2,
                        double eps, double weight_decay, double l1, double l2, int32_t step, void* stream);

/* inr_train_step and inr_adam_step as ONE call for single-rank steps (nothing sits between the reduction and the
 * update): the Adam update and the re-pack ride in the slab reduction's launch (flat-layout plans: SIREN / FFN, fp32 and
 * bf16; two launches otherwise) -- one launch and one pass over the gradient less per step.  Bit-identical to the two
 * calls; `grads` still receives the gradient. */
int inr_train_adam_step(const inr_plan* plan, const inr_loss_desc* loss, float* params, float* packed,
                        const float* x, const float* enc_B, const float* gt, const uint8_t* mask, int64_t B,
                        const inr_workspace* ws, float* grads, float* loss_out, float* exp_avg,
                        float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double l1, double l2, int32_t step, void* stream);

/* The same update with the step count in DEVICE memory, so that the launch carries no argument that changes from
 * one step to the next and a whole step (inr_train_step + this) can be captured once in a HIP graph and replayed:
 * `step_dev` holds the number of steps taken so far (t); the kernel reads (step_size, bc2_sqrt) from
 * `sched[2*min(t, n_sched-1)]` — device copy of a table made by inr_adam_schedule — and a one-thread kernel behind it
 * stores t + 1.  Results are bit-identical to inr_adam_step(step = t + 1) while t < n_sched; with beta1 = 0.9,
 * beta2 = 0.999 both fp32 terms have converged after 16 600 steps, so a table of 32 768 entries is exact for any run
 * length.  A new learning rate (the per-epoch LambdaLR of train.py:153,251) means a new table, not a new graph. */
int inr_adam_step_dev(const inr_plan* plan, float* params, const float* grads, float* exp_avg,
                      float* exp_avg_sq, float* packed, const float* sched, int32_t n_sched,
                      int32_t* step_dev, double beta1, double beta2, double eps, double weight_decay,
                      double l1, double l2, void* stream);
/* Host helper: host_out[2*t] = float(lr / (1 - beta1^(t+1))), host_out[2*t+1] = float(sqrt(1 - beta2^(t+1))),
 * t = 0..n-1, in the doubles torch.optim.Adam uses (the same code path as inr_adam_step).  No GPU work. */
int inr_adam_schedule(double lr, double beta1, double beta2, int32_t n, float* host_out);

/* (v7 addition) Image metrics of the validation epoch (train.py:221-231): replaces fastmri.complex_abs + fastmri.rss and
 * models/utils.py:227-250 (psnr; ssim = skimage.metrics.structural_similarity of scikit-image 0.18.1).
 * `coils` [C,H,W,2] = the coil images after the inverse FFT (the network outputs themselves in image-space configs);
 * rss_out [H,W] = sqrt(sum_c |z_c|^2), |z| = sqrt(re^2 + im^2), in fp32 and fixed coil order.  `ref` [H,W] (the
 * ground-truth RSS image) may be NULL: RSS only, and metrics_out / scratch are not touched (may be NULL).  Otherwise
 * metrics_out[8] (fp64, device) = psnr, ssim, sse, max_ref, min_ref, max_rec, min_rec, data_range, where
 *   psnr = 10 log10(max_ref / (sse / (H W) + 1e-10))  (max, not max^2, as the reference),
 *   data_range = max(max_ref, max_rec) - min(min_ref, min_rec) in fp32,
 *   ssim = mean over the interior (3-pixel crop) of the 7x7 uniform-window SSIM of the images cast to fp64, K1 = 0.01,
 *          K2 = 0.03, sample covariance; NaN when data_range == 0.
 * H or W < 7 with a reference is INR_ERR_INVALID (skimage raises).  `scratch` = scratch_doubles fp64 words, at least
 * what inr_image_metrics_scratch gives for (C, H, W).  No atomics, no host synchronisation: three launches on `stream`,
 * bitwise reproducible, capturable in a graph. */
int inr_image_metrics_scratch(int64_t C, int64_t H, int64_t W, int64_t* scratch_doubles);
int inr_image_metrics(const float* coils, int64_t C, int64_t H, int64_t W, const float* ref, float* rss_out,
                      double* metrics_out, double* scratch, int64_t scratch_doubles, void* stream);

/* (v7 addition) One shuffled epoch (no reference counterpart beyond the shuffle=True its callers pass and its loaders
 * drop, train.py:281,307 against models/utils.py:84-99): output row j is input row order(j), the keyed stateless
 * permutation of DESIGN.md section 4.12 -- a pure function of (n, seed, epoch), restated in numpy by
 * inr_mi355x/shuffle.py::epoch_order with the same 32-bit integers.  1 <= n < 2^31.
 *   coords [n,3] -> coords_out, gt [n,2] -> gt_out (8-byte aligned), dist [n] -> dist_out, mask [n] u8 -> mask_out:
 *     each pair is optional (both NULL) and must not alias; mask may come without mask_out (counts only);
 *   batch_counts (int32, ceil(n / batch_size) entries; may be NULL): sampled rows (mask != 0; every row without a mask)
 *     among output rows [b * batch_size, (b + 1) * batch_size) -- integer atomics on words the call zeroes first, exact;
 *   order_out (int64 [n]; may be NULL): order(j) itself.
 * One memset node (batch_counts only) and one kernel launch on `stream`; nothing is allocated, nothing is read back. */
int inr_shuffle_epoch(int64_t n, int64_t batch_size, uint64_t seed, uint32_t epoch, const float* coords,
                      const float* gt, const float* dist, const uint8_t* mask, float* coords_out, float* gt_out,
                      float* dist_out, uint8_t* mask_out, int32_t* batch_counts, int64_t* order_out, void* stream);

/* (v7 additions) Weighted epochs (no reference counterpart beyond the per-ring loss weights of
 * train_variations/train_weighted_kspace.py and HDRLoss_FF.forward(..., weights=)): the rows of an
 * epoch drawn with probability proportional to a per-row weight, so that the unweighted step's expected gradient is that
 * of the weighted loss.  Integer arithmetic after one fp64 product per row: results do not depend on a summation order
 * or a launch shape, and inr_mi355x/sampling.py (row_cdf_numpy, epoch_draw_numpy) restates them bit for bit.
 *
 * inr_row_cdf: w [n] device fp32, mask [n] device uint8 or NULL, scale an fp64 argument, cdf_out [n] device uint64.
 *   ticks q_i = 0 where mask[i] == 0 or w_i is NaN, negative or +-0; otherwise min(2^32 - 1, floor(fp64(w_i) * scale)),
 *   so +inf gives 2^32 - 1.  cdf_out[i] = q_0 + ... + q_i (inclusive; fits for n < 2^31).
 *   Three launches on `stream`: per-tile sums, one workgroup over the tile sums in `scratch`, per-tile scan plus offset.
 *   No workgroup waits on another.  scratch: uint64 words, their number from inr_row_cdf_scratch.  16-byte loads of w
 *   and stores of cdf_out when both are 16-byte aligned (and mask 4-byte aligned).  Nothing is allocated or read back.
 *   INR_ERR_INVALID before any launch: a null w, cdf_out or scratch; n < 1 or n >= 2^31; scale not finite or <= 0;
 *   scratch_words below the query's; w not 4-byte or cdf_out / scratch not 8-byte aligned; cdf_out or scratch
 *   overlapping another buffer.
 *
 * inr_sample_epoch: cdf [n] as above, m output rows, 1 <= n, m < 2^31.  With T = cdf[n-1] (read by the kernel) and
 *   stride = T div m, output position j holds stratum s = order_m(j) -- inr_shuffle_epoch's permutation for (seed, epoch)
 *   over [0, m) -- whose threshold is t_s = s * stride + (u_s mod stride), u_s = MIX(s ^ k0) * 2^32 + MIX(s ^ k1) under two
 *   keys made from (seed, epoch) by the key schedule with the constant 0x85EBCA6B.  The row is the smallest i with
 *   cdf[i] > t_s (binary search, at most 31 steps).  A row without ticks is never drawn; row i is drawn between
 *   max(0, floor(q_i / stride) - 1) and floor(q_i / stride) + 2 times when T mod m < stride (the strata cover
 *   [0, m * stride): the last T mod m ticks are never reached); equal ticks and m == n give the shuffle's order itself.
 *   stride == 0 (T < m): every position takes the row of threshold 0, row 0 when T == 0 -- defined, not useful.
 *   The buffers from `coords` on follow inr_shuffle_epoch: inputs have n rows, outputs m rows, batch_counts
 *   ceil(m / batch_size) entries; one memset node (batch_counts only) and one launch.
 *   INR_ERR_INVALID before any launch: a null or misaligned cdf; n or m outside [1, 2^31); and inr_shuffle_epoch's buffer
 *   rules with its messages. */
int inr_row_cdf_scratch(int64_t n, int64_t* scratch_words);
int inr_row_cdf(const float* w, const uint8_t* mask, int64_t n, double scale, uint64_t* cdf_out, uint64_t* scratch,
                int64_t scratch_words, void* stream);
int inr_sample_epoch(const uint64_t* cdf, int64_t n, int64_t m, int64_t batch_size, uint64_t seed, uint32_t epoch,
                     const float* coords, const float* gt, const float* dist, const uint8_t* mask, float* coords_out,
                     float* gt_out, float* dist_out, uint8_t* mask_out, int32_t* batch_counts, int64_t* order_out,
                     void* stream);

/* (v7 additions) The pictures and the per-coil table of the validation epoch (train.py:221-238, models/utils.py:254-287).
 * All three: no atomics, fixed-order two-stage reductions (bitwise reproducible), no host synchronisation, nothing
 * allocated, capturable in a graph; scratch is the caller's, its size comes from the matching *_scratch query.
 *
 * inr_kspace_display -- the is_kspace branch of save_im (models/utils.py:262-267) in fp32: `coils` [C,H,W,2]; `minus`
 * [C,H,W,2] or NULL (non-NULL: the input is coils - minus, the error picture of train.py:225); both 8-byte aligned.
 *   g = sqrt(sum_c |z_c|^2), |z| = sqrt(re^2 + im^2);  g *= expm1(smoothing_factor) / max(g);  g = log1p(g);
 *   out [H,W] = g / max(g), in 0..1.
 * max propagates NaN (torch.max).  An all-zero input gives NaN in every pixel, as the reference's 0 * (expm1(sf) / 0) does.
 * Three launches on `stream`; scratch = scratch_floats fp32 words.
 *
 * inr_gray8 -- the byte plt.imsave(..., format="png", cmap="gray") stores in the R (= G = B) channel for img [H,W]:
 *   x = |img| when take_abs (save_im's np.abs, models/utils.py:257,260), else img;
 *   vmin, vmax = the arguments when has_range != 0 (vmin <= vmax, else INR_ERR_INVALID), else the extrema of the finite x;
 *   n = (x - vmin) / (vmax - vmin) in fp32, n = 0 everywhere when vmax == vmin (a constant picture is all zeros);
 *   index = min(floor(256 n), 255), 0 for n < 0, 255 for n > 1;  out [H,W] uint8 = lut[index].
 * `lut` = 256 device bytes, matplotlib's table for the 'gray' map -- uint8(trunc(i * (1 / 255) * 255)) in float64, which is
 * NOT the identity (i - 1 at i = 33, 37, 41, ...); the caller uploads it once.  Non-finite pixels are masked by
 * matplotlib: byte 0 here, NaN in norm_out.  norm_out [H,W] fp32 (may be NULL) receives n.  scratch (scratch_floats fp32
 * words) is only touched when has_range == 0 and may be NULL otherwise.  One launch with a range, two without.
 *
 * inr_coil_stats -- stats_per_coil (models/utils.py:274-283): coils [C,H,W,2] (8-byte aligned, C <= 65535) ->
 * stats [C,4] fp64 = mean, std (unbiased, n - 1: torch.Tensor.std's default), max, min over the 2 H W values of each
 * coil.  Sums are accumulated in fp64, the deviations in a second pass from the fp64 mean; max / min are exact.  Inputs
 * are taken as finite.  Three launches; scratch = scratch_doubles fp64 words. */
int inr_kspace_display_scratch(int64_t C, int64_t H, int64_t W, int64_t* scratch_floats);
int inr_kspace_display(const float* coils, const float* minus, int64_t C, int64_t H, int64_t W, float smoothing_factor,
                       float* out, float* scratch, int64_t scratch_floats, void* stream);
int inr_gray8_scratch(int64_t H, int64_t W, int64_t* scratch_floats);
int inr_gray8(const float* img, int64_t H, int64_t W, int32_t take_abs, int32_t has_range, float vmin, float vmax,
              const uint8_t* lut, uint8_t* out, float* norm_out, float* scratch, int64_t scratch_floats, void* stream);
int inr_coil_stats_scratch(int64_t C, int64_t H, int64_t W, int64_t* scratch_doubles);
int inr_coil_stats(const float* coils, int64_t C, int64_t H, int64_t W, double* stats, double* scratch,
                   int64_t scratch_doubles, void* stream);

/* (v7 addition) Rows of a coordinate grid, made on the device (replaces create_coords, data/utils.py:98-108, and the
 * upload of its result).  Row r = (k H + y) W + x of the flattened (k, y, x) grid is
 *   (v(coils[k]; -1, 1, coils_total), v(y; y0, y1, H), v(x; x0, x1, W)),  dist = sqrt(y^2 + x^2)  (y, x: the values),
 *   v(i; a, b, n) = a when n == 1, else a + step i for i < n / 2 and b - step (n - 1 - i) for the rest,
 *   step = (b - a) / (n - 1),
 * everything in fp32, every operation rounded on its own (no FMA), the square root correctly rounded: a pure function
 * of its arguments, restated in numpy by inr_mi355x/grid.py::grid_rows_numpy.  It is NOT torch.linspace bit for bit
 * (whose CPU values depend on the host's vector width); the two differ by at most 2^-24 on [-1, 1].
 *   coords [n_rows,3] and dist [n_rows] (may be NULL) receive rows [row_lo, row_lo + n_rows) of the
 *   n_coils * H * W rows, and nothing behind them; 0 <= n_rows < 2^31 per call, the grid's total is int64;
 *   n_rows == 0 succeeds without a launch.  16-byte aligned buffers are written with 16-byte stores.
 * INR_ERR_INVALID before any launch: null g / coords; H, W, n_coils or coils_total < 1; n_coils > 64; a coil index
 * outside [0, coils_total); a non-finite window bound; negative or out-of-range rows.
 * One kernel launch on `stream`; nothing is allocated, nothing is read back; capturable in a graph. */
typedef struct {
  int32_t coils_total;    /* C of the fit: the coil axis is v(c; -1, 1, C) */
  int32_t n_coils;        /* which coils, in output order */
  int32_t coils[64];
  int32_t H, W;           /* points per axis of the rendered grid */
  float y0, y1, x0, x1;   /* window; the fit's own grid is -1, 1, -1, 1 */
} inr_grid_desc;
int inr_grid_rows(const inr_grid_desc* g, int64_t row_lo, int64_t n_rows, float* coords, float* dist, void* stream);

/* (v7 addition) Radial band statistics of an [n,2] field in one pass (replaces the per-ring masked reductions of
 * clustering.py:48-61, 100-135; the per-ring report of the validation epoch has no reference counterpart; DESIGN.md
 * section 4.17).  dist [n], gt [n,2], pred [n,2] (may be NULL), mask [n] uint8 (may be NULL): device.  band_lo / band_hi:
 * HOST arrays of n_bands floats.  Row i belongs to band b iff band_lo[b] <= dist[i] <= band_hi[b], compared in fp32 with
 * both ends included; bands may overlap, nest, be empty or leave rows uncovered.  With `mask`, only rows with
 * (mask[i] != 0) == (mask_select != 0) take part.  stats [n_bands][INR_BAND_FIELDS] (fp64, device), per band:
 *   n         rows in the band
 *   energy    sum of gt_re^2 + gt_im^2
 *   sse       sum of |pred - gt|^2                                   (0 without pred)
 *   max_abs2  max of fl32(fl32(re re) + fl32(im im)) of gt
 *   max_comp  max of |gt component| over both components
 *   min_comp  min of |gt component| over both components
 *   max_err2  max of |pred - gt|^2                                   (-inf without pred)
 * A sum term is (double)a * (double)a + (double)b * (double)b (a, b = the components, or the fp64 differences of the
 * components), every operation rounded on its own, and the terms are added in fp64 in a fixed order; the extrema are
 * exact.  An empty band has n = 0, sums 0, maxima -inf, minima +inf.  Inputs are taken as finite (a NaN dist is in no
 * band).  inr_mi355x/bands.py::band_stats_numpy restates this in numpy.
 * INR_ERR_INVALID before any launch: a null dist / gt / bounds / stats / scratch; n < 1 or n >= 2^31; n_bands outside
 * 1..INR_BAND_MAX; a NaN bound or band_lo[b] > band_hi[b].
 * `scratch` = at least the fp64 words inr_band_stats_scratch gives for (n, n_bands) -- a function of its arguments
 * alone.  Two launches on `stream` (workgroup partials, then one block per band); no atomics, fixed-order reductions:
 * two calls on the same inputs give the same bits.  Nothing is allocated, nothing is read back, capturable in a graph.
 * 16-byte aligned dist / gt / pred (mask: 4-byte) are read with 16-byte loads, INR_BAND_TILE_ROWS rows per workgroup
 * and step. */
#define INR_BAND_MAX 64
#define INR_BAND_FIELDS 7
#define INR_BAND_TILE_ROWS 1024
int inr_band_stats_scratch(int64_t n, int32_t n_bands, int64_t* scratch_doubles);
int inr_band_stats(const float* dist, const float* gt, const float* pred, const uint8_t* mask, int32_t mask_select,
                   int64_t n, const float* band_lo, const float* band_hi, int32_t n_bands, double* stats,
                   double* scratch, void* stream);

/* (v7 addition) Per-ring scaling of an [n,2] field (the reference's scale_space,
 * train_variations/train_normalize_per_bucket.py:20-27).  dist [n], in [n,2], out [n,2]: device
 * fp32.  radii [n_rings+1], divisors [n_rings]: HOST arrays; they travel as kernel arguments.  Row i belongs to ring r
 * iff radii[r] <= dist[i] < radii[r+1], compared in fp32, lower end included and upper end excluded.  Both components
 * of a row in ring r become in / divisors[r], one correctly rounded fp32 division each.  A row in no ring (dist below
 * radii[0], at or above radii[n_rings], or NaN) is copied unchanged, bit for bit.  Equal neighbouring radii make an
 * empty ring; a row at that radius falls into the next non-empty one.  The inverse is the same call with the table
 * fl32(1 / divisors[r]).  inr_mi355x/ringnorm.py::ring_scale_numpy restates this in numpy.
 * out == in (in place) is allowed.  One launch on `stream`; no scratch, nothing is allocated, nothing is read back,
 * capturable in a graph.  Four rows per lane, with 16-byte loads and stores when dist, in and out are 16-byte aligned;
 * nothing is written at or beyond row n.
 * INR_ERR_INVALID before any launch: a null pointer; n < 1 or n >= 2^31; n_rings outside 1..INR_BAND_MAX; a NaN radius;
 * radii that decrease; a divisor that is zero, NaN or infinite; in / out not 8-byte aligned or dist not 4-byte aligned;
 * out overlapping in other than out == in, or overlapping dist. */
int inr_ring_scale(const float* dist, const float* in, float* out, int64_t n, const float* radii, const float* divisors,
                   int32_t n_rings, void* stream);

/* (v7 addition) Continuous radial scaling of an [n,2] field (no reference counterpart): the
 * divisor of a ring-normalised fit without its jumps at the ring edges.  dist [n], in [n,2], out [n,2], profile
 * [n_knots]: device fp32.  The profile is piecewise linear on n_knots uniform knots that start at r_lo and lie
 * 1 / inv_step apart, and constant beyond both ends.  Per row, every line one correctly rounded fp32 operation, nothing
 * contracted into an FMA:
 *   s  = d - r_lo;   u = s * inv_step;   u = u < 0 ? 0 : (u > n_knots-1 ? n_knots-1 : u)
 *   k  = min((int)u, n_knots - 2);   t = u - (float)k          (exact)
 *   df = p[k+1] - p[k];   pr = t * df;   q = p[k] + pr
 *   out = multiply ? in * q : in / q                           (both components; a true division)
 * A row whose dist is NaN is copied unchanged, bit for bit.  The inverse of a division is the same call on the same
 * profile with multiply != 0.  inr_mi355x/ringnorm.py::radial_scale_numpy restates this in numpy.
 * out == in (in place) is allowed.  One launch on `stream`; no scratch, nothing is allocated, nothing is read back,
 * capturable in a graph.  Every workgroup stages the profile in LDS; four rows per lane, with 16-byte loads and stores
 * when dist, in and out are 16-byte aligned; nothing is written at or beyond row n.
 * INR_ERR_INVALID before any launch: a null pointer; n < 1 or n >= 2^31; n_knots outside 2..INR_RADIAL_KNOTS_MAX; a NaN
 * or infinite r_lo; an inv_step that is not finite and positive; in / out not 8-byte aligned, dist or profile not 4-byte
 * aligned; out overlapping in other than out == in, or overlapping dist or profile.  The profile's values are device
 * data and are not checked. */
#define INR_RADIAL_KNOTS_MAX 4096
int inr_radial_scale(const float* dist, const float* in, float* out, int64_t n, const float* profile, int32_t n_knots,
                     float r_lo, float inv_step, int32_t multiply, void* stream);

/* (v7 additions) A learned radial gain (the reference's ScalerWrapper, models/networks.py:380-405: res = backbone(x) *
 * exp(-scaler(z))).  y [B,2] is the backbone's output, s [B] the gain network's, both from
 * inr_forward; the gradients go back through inr_backward of either plan.  Per row, in fp32:
 *   g = expf(-s);  res_c = y_c g;  (loss, dres) = the pointwise loss of inr_loss_grad on (res, gt);
 *   dy_c = dres_c g;  ds = -(dres_0 res_0 + dres_1 res_1).
 * inr_gain_loss_grad: every loss kind inr_loss_grad takes, the same inr_loss_desc (inv_count = 1 / sampled rows, hdr_A).
 *   Rows with mask[r] == 0 (mask may be NULL: every row) get dy = ds = 0 and stay out of the loss; res (may be NULL) is
 *   written for every row.  loss_out[0] = the loss; loss_out[1..256] are ordered partial sums (a loss_out buffer holds
 *   INR_LOSS_WORDS floats), folded by one thread: no atomics, the same inputs give the same bits on every call, and
 *   res == NULL changes no bit of the other outputs.  y, gt, dy, res 8-byte aligned, s, ds 4-byte aligned; with 16- and
 *   8-byte alignment two rows move per 16-byte access, and the results do not depend on which path ran.
 *   Two launches on `stream`.
 * inr_gain_apply: res = y exp(-s) alone (no-grad sweeps), equal bit for bit to inr_gain_loss_grad's res; res == y is
 *   allowed.  One launch.
 * INR_ERR_INVALID before any launch: a null loss, y, s, gt, loss_out, dy, ds (res in inr_gain_apply); B <= 0; an unknown
 * loss kind; a misaligned pointer. */
int inr_gain_loss_grad(const inr_loss_desc* loss, const float* y, const float* s, const float* gt, const uint8_t* mask,
                       int64_t B, float* res, float* loss_out, float* dy, float* ds, void* stream);
int inr_gain_apply(const float* y, const float* s, int64_t B, float* res, void* stream);

/* (v7 additions) A mixture of heads (the reference's MultiHeadWrapper with backbone = None, models/networks.py:275-328;
 * DESIGN.md section 4.27): K expert networks' outputs y_k [B,2] mixed by a gate network's w [B,K], all from inr_forward;
 * the gradients go back through inr_backward of each plan.  Per row, in fp32, every product and sum rounded on its own
 * (nothing contracted), d = dist[row], t = gt[row]:
 *   pre_c = ((w_0 y_0c + w_1 y_1c) + ...) + w_{K-1} y_{K-1,c};   res_c = clamp ? min(max(pre_c, -1), 1) : pre_c
 *   (L_0, dres) = the pointwise loss of inr_loss_grad on (res, t) with inv_count[0]
 *   dpre_c = dres_c where clamp == 0 or -1 <= pre_c <= 1 (both ends included), else 0
 *   dw_k = dpre_0 y_k0 + dpre_1 y_k1
 *   where radii[k] <= d <= radii[k+1] (both ends included; a row on an edge is in two rings):
 *       (L_{1+k}, g_k) = the same pointwise loss on (y_k, t) with inv_count[1+k];  elsewhere g_k = 0
 *   dy_kc = g_kc (detach != 0)  or  g_kc + w_k dpre_c (detach == 0)
 * inr_mix_loss_grad: the loss kinds inr_gain_loss_grad takes; the descriptor's inv_count is replaced per term by
 *   mix->inv_count (the mixed term, then rings 0..K-1; 0 for a ring without rows), its hdr_A serves every term.  Rows with
 *   mask[r] == 0 (mask may be NULL: every row) get dy_k = dw = 0 and stay out of every term; res (may be NULL) is written
 *   for every row, and whether it is changes no bit of the other outputs.  loss_out[0] = the total, loss_out[1 .. K+1] =
 *   the mixed term and the K ring terms; loss_out[INR_MIX_PARTIALS + term * INR_MIX_BLOCKS + block] are ordered partial
 *   sums (a loss_out buffer holds INR_LOSS_WORDS floats), each term folded by one thread in block order and the total
 *   added in term order: no atomics, the same inputs give the same bits on every call.  mix->y[k] / mix->dy[k], k <
 *   n_heads: expert k's [B,2] buffers (no stacked copy is made); dw [B,K] is the gate plan's dout.  y_k, dy_k, gt, res
 *   8-byte aligned, w, dw, dist 4-byte aligned; with 16-byte alignment throughout two rows move per 16-byte access, and
 *   the results do not depend on which path ran.  Two launches on `stream`.
 * inr_mix_apply: res alone (no-grad sweeps; reads n_heads, clamp and y of the descriptor), equal bit for bit to
 *   inr_mix_loss_grad's res; res == y[0] is allowed.  One launch.
 * INR_ERR_INVALID before any launch, the outputs untouched: a null loss, mix, w, gt, dist, loss_out or dw (mix, w, res in
 * inr_mix_apply); n_heads outside 2..INR_MIX_MAX_HEADS; a null y[k] or dy[k] below n_heads; radii that do not increase
 * (or a NaN among them); a negative or non-finite inv_count; B < 1; a loss kind outside inr_gain_loss_grad's; a
 * misaligned pointer. */
#define INR_MIX_MAX_HEADS 8
#define INR_MIX_BLOCKS 55
#define INR_MIX_PARTIALS 10
typedef struct {
  int32_t n_heads, detach, clamp, reserved;
  float radii[INR_MIX_MAX_HEADS + 1];
  float inv_count[INR_MIX_MAX_HEADS + 1];
  const float* y[INR_MIX_MAX_HEADS];
  float* dy[INR_MIX_MAX_HEADS];
} inr_mix_desc;
int inr_mix_loss_grad(const inr_loss_desc* loss, const inr_mix_desc* mix, const float* w, const float* gt,
                      const float* dist, const uint8_t* mask, int64_t B, float* res, float* loss_out, float* dw,
                      void* stream);
int inr_mix_apply(const inr_mix_desc* mix, const float* w, int64_t B, float* res, void* stream);

/* (v7 additions) SENSE-model fits (no reference counterpart): two networks in IMAGE space, fitted to
 * k-space data.  img [H*W,2] is the image network's output (one complex number per pixel), sens [G*H*W,2] the
 * sensitivity network's for G coils, both from inr_forward; x / gx [G,H,W,2] the coil images and the gradient that came
 * back to them (through the caller's FFT and inr_loss_grad); dimg / dsens like img / sens, for inr_backward of either
 * plan.  A (re, im) pair is one complex number.  Per pixel p = (y, x) and coil g, in fp32, every product and sum rounded
 * on its own (nothing contracted), in this order:
 *   inr_sense_apply:  re = sr*ir - si*ii;  im = sr*ii + si*ir;  x[g][q] = (scale*re, scale*im)
 *   inr_sense_grad:   (gr, gi) = gx[g][q];  ur = scale*gr;  ui = scale*gi
 *                     dsens[g][p] = (ir*ur + ii*ui, ir*ui - ii*ur)
 *                     dimg[p]     = (((0 + t_0) + t_1) + ...) + t_{G-1},  t_g = (sr*ur + si*ui, sr*ui - si*ur)
 * shift = 0: q = p.  shift = 1: q = ((y - H/2) mod H, (x - W/2) mod W) with integer H/2, W/2 -- where torch.fft.ifftshift
 * over (H, W) puts pixel p, for every parity of H and W -- so that a plain 2-D FFT of x is the centred transform of the
 * coil images before its fftshift, and no shifted copy is made in a step.
 * One lane owns its pixel(s) for every coil: no atomics, no shared-memory or cross-lane reduction, the same bits on every
 * call.  With every pointer 16-byte aligned and W and W/2 even, two pixels move per 16-byte access, else one per 8-byte
 * access; the results do not depend on which path ran.  One launch on `stream`, sized from H * W.
 * INR_ERR_INVALID before any launch, the outputs untouched: a null pointer; G, H or W < 1 (or H, W > 2^30, G*H*W > 2^40);
 * shift outside {0, 1}; a non-finite scale; a pointer that is not 8-byte aligned; an output that overlaps an input or
 * the other output. */
int inr_sense_apply(const float* img, const float* sens, int32_t G, int64_t H, int64_t W, float scale, int32_t shift,
                    float* x, void* stream);
int inr_sense_grad(const float* img, const float* sens, const float* gx, int32_t G, int64_t H, int64_t W, float scale,
                   int32_t shift, float* dimg, float* dsens, void* stream);

/* (v7 additions) SENSE fits on calibrated coil maps (no reference counterpart): the maps come once
 * from the fully sampled centre of k-space, and a step needs the image half of inr_sense_grad alone.  Every product, sum,
 * division and square root below is one correctly rounded fp32 operation (nothing contracted), sums start from zero;
 * no atomics, the same bits on every call.  A (re, im) pair is one complex number; a complex product u * v is
 * p0 = ur*vr; p1 = ui*vi; p2 = ur*vi; p3 = ui*vr; (p0 - p1, p2 + p3).
 *   inr_sense_lowres:  kc [C,a,b,2] the (windowed) centre block of the centred k-space, ey [a,Ho,2] / ex [b,Wo,2] the
 *       phasor tables of the Ho row and Wo column positions (made on the host in float64 with the phase reduced first,
 *       carrying 1/sqrt(H) and 1/sqrt(W); the kernel evaluates no sine or cosine), out [C,Ho,Wo,2]:
 *         T[c][j][x] = sum_i kc[c][j][i] * ex[i][x] (i ascending);  out[c][y][x] = sum_j ey[j][y] * T[c][j][x] (j ascending)
 *       On the fit's own grid that is the centred orthonormal inverse transform of the zero-padded block; other positions
 *       interpolate it exactly.
 *   inr_sense_maps:  low [C,P,2] -> rss [P], maps [C,P,2].  r2 = sum_c (re*re + im*im) in coil order, rss[p] = sqrtf(r2),
 *       maps[c][p] = low[c][p] / rss[p] where rss[p] > floor * max_p rss[p] and rss[p] > 0, else (0, 0).  Two launches:
 *       the first writes rss, in the second every workgroup takes the (exact) maximum of rss before it divides.
 *   inr_sense_adjoint:  sens [G,H*W,2], gx [G,H,W,2] -> dimg [H*W,2]: the dimg of inr_sense_grad on the same inputs, bit
 *       for bit (same operations per pixel, same coil order, same place q under `shift`, same two-pixel rule); it reads
 *       no img and writes no dsens.
 * INR_ERR_INVALID before any launch, the outputs untouched: a null pointer; a or b outside 2..INR_SENSE_CALIB_MAX; C outside
 * 1..65535, Ho or Wo outside 1..2^20 (lowres); C, P, G, H or W < 1 or more than 2^40 complex numbers; floor outside
 * [0, 1); shift outside {0, 1}; a non-finite scale; a pointer that is not 8-byte aligned (rss: 4-byte); an output that
 * overlaps an input or the other output. */
#define INR_SENSE_CALIB_MAX 64
int inr_sense_lowres(const float* kc, const float* ey, const float* ex, int32_t C, int32_t a, int32_t b, int64_t Ho,
                     int64_t Wo, float* out, void* stream);
int inr_sense_maps(const float* low, int32_t C, int64_t P, float floor, float* maps, float* rss, void* stream);
int inr_sense_adjoint(const float* sens, const float* gx, int32_t G, int64_t H, int64_t W, float scale, int32_t shift,
                      float* dimg, void* stream);

/* (v7 addition) A total-variation prior on the IMAGE of a SENSE fit (no reference counterpart; the
 * reference's tv_loss, inr_loss_tv_grad here, is on a coil's predicted k-space).  img [H,W,2] is one complex image (the
 * image network's output, a (re, im) pair per pixel), dimg like it.  Smoothed isotropic TV with forward differences that
 * are zero past the last row / column; per pixel p = (y, x), in fp32, every product, sum, difference, square root and
 * division rounded on its own (nothing contracted), in this order:
 *   ax = I[y][x+1] - I[y][x];  ay = I[y+1][x] - I[y][x]          (per component; 0 where x = W-1 / y = H-1)
 *   s0 = axr*axr; s1 = axi*axi; s2 = ayr*ayr; s3 = ayi*ayi;  a = s0 + s1;  b = s2 + s3;  q0 = a + b;  q = q0 + e2
 *   n = sqrtf(q)  (e2 = eps*eps);   u = ax / n;  v = ay / n      (both (0, 0) where n == 0, which only eps == 0 can give)
 *   term = n - eps
 *   t0 = u(y, x-1) - u(p);  t1 = v(y-1, x) - v(p);  t = t0 + t1;  d = c * t        (a missing neighbour's u / v is 0)
 *   c = weight / (H W), formed in fp64 and rounded to fp32 once
 * dimg[p] = d when accumulate == 0, dimg[p] + d (one fp32 sum per component) when accumulate == 1; dimg may be NULL (the
 * value alone; whether it is changes no bit of loss_out[0]).  loss_out[0] = S * (weight / (H W)) formed in fp64 and rounded
 * once -- written, not added -- where S is the fp64 sum of the fp32 terms: a lane's terms in the order it meets them, the
 * 256 lanes of a block by a fixed tree, the blocks' partials in block order by one thread of a second launch.
 * loss_out must be 8-byte aligned; loss_out[1] is unused and loss_out[INR_IMAGE_TV_PARTIALS + 2 b], b < the launch's
 * block count <= INR_IMAGE_TV_BLOCKS, holds block b's fp64 partial: words 2 .. 511 are scratch, and a buffer of
 * INR_LOSS_WORDS floats serves.  A gather: one lane owns a pixel (two neighbouring pixels where W is even: one 16-byte
 * access when img and dimg are 16-byte aligned, two of 8 bytes otherwise) and recomputes n at its own pixel, its left and
 * its upper neighbour.  No atomics: the same inputs give the same bits on every call, whatever the alignment.  Two
 * launches on `stream`.
 * INR_ERR_INVALID before any launch, the outputs untouched: a null img or loss_out; H or W < 1 (or > 2^30, or H * W > 2^40);
 * eps negative or not finite; weight not finite; accumulate outside {0, 1}; img or dimg not 8-byte aligned, loss_out not
 * 8-byte aligned; dimg or loss_out overlapping img or each other. */
#define INR_IMAGE_TV_BLOCKS 255
#define INR_IMAGE_TV_PARTIALS 2
int inr_image_tv_grad(const float* img, int64_t H, int64_t W, float weight, float eps, int32_t accumulate,
                      float* loss_out, float* dimg, void* stream);

/* inr_focal_loss_grad (below): its descriptor, its block count and where the words of its loss_out buffer lie */
#define INR_FOCAL_BLOCKS 255
#define INR_FOCAL_PARTIALS 1   /* loss_out[1 .. 255] */
#define INR_FOCAL_MAXIMA 256   /* loss_out[256 .. 510] */
#define INR_FOCAL_NMAX 511     /* the last of the INR_LOSS_WORDS words */
typedef struct { float alpha; int32_t log_matrix; float loss_weight; float inv_count; } inr_focal_desc;
/* (v7 addition) The focal frequency loss (the reference's FocalFrequencyLoss.loss_formulation with matrix = None,
 * metrics/losses.py:57-119; Jiang et al., ICCV 2021) on k-space rows out, gt [B,2]: every sampled
 * row's squared error weighted by that error relative to the largest of the batch.  Per sampled row r (mask[r] != 0; mask
 * may be NULL: every row), every fp32 operation rounded on its own (no contraction), inv = inv_count = 1 / sampled rows:
 *   e_o = out_o - gt_o;  q = e_0 e_0 + e_1 e_1;  m = sqrtf(q) (alpha == 1) or powf(sqrtf(q), alpha);
 *   n = logf(m + 1.0f) (log_matrix != 0) or m;      n_max = the largest n of the sampled rows (0 when there are none);
 *   w = 0 if n_max == 0, else fminf(fmaxf(n / n_max, 0), 1)          -- a constant: no gradient flows through w
 *   loss_out[0] = ((sum_r w_r q_r) inv) loss_weight                  -- the sum in the order given below, then two products
 *   dout_o = (((loss_weight 2) e_o) w) inv                           -- in this order: the product by 2 is exact, so the
 *            row that attains n_max (w == 1.0f exactly: both passes evaluate n with one device function) gets
 *            fl(fl(loss_weight 2 e_o) inv) to the bit.  Rows with mask[r] == 0: dout = 0, not in n_max, not in the sum.
 * n_max == 0 (prediction equals target on every sampled row, or nothing is sampled) gives loss 0 and dout 0, never NaN.
 * dout may be NULL (the loss alone); whether it is changes no bit of loss_out.  Non-finite inputs are outside the contract.
 * Two passes over INR_FOCAL_BLOCKS contiguous ranges of row pairs: the first leaves every range's largest n in
 * loss_out[INR_FOCAL_MAXIMA + b]; the second folds those words itself (every block, the same fixed tree; block 0 stores
 * n_max in loss_out[INR_FOCAL_NMAX]), writes dout and leaves its ordered partial sum of w q in loss_out[INR_FOCAL_PARTIALS
 * + b] (a lane's rows in order, the 256-lane tree); one thread folds the partials in block order.  No atomics: the same
 * inputs give the same bits on every call.  A max does not depend on order, so n_max is exact.  loss_out holds
 * INR_LOSS_WORDS floats.  out, gt, dout 8-byte aligned; with 16-byte alignment two rows move per 16-byte access and the
 * results do not depend on which path ran.  Three launches on `stream`.
 * INR_ERR_INVALID before any launch, the outputs untouched: a null d, out, gt or loss_out; B <= 0; alpha <= 0 or a
 * non-finite alpha, loss_weight or inv_count; out, gt or dout not 8-byte aligned. */
int inr_focal_loss_grad(const inr_focal_desc* d, const float* out, const float* gt, const uint8_t* mask,
                        int64_t B, float* loss_out, float* dout, void* stream);

/* (v7 addition) Software coil compression (no reference counterpart).  A scan is coil-major:
 * data [C][N][2], complex fp32 (re, im) pairs, N = H*W pixels per coil.
 * inr_coil_gram: gram [C][C][2] (fp64, device, both triangles), G[i][j] = sum_p x_i[p] conj(x_j[p]).  Every product is
 * formed in fp64 from the fp32 inputs (exact) and every sum is fp64; the order of the sums is fixed (workgroup partials in
 * `scratch`, then one block per pair; no atomics), so two calls on the same input give the same bits.  G[j][i] is
 * written as the conjugate of G[i][j] and the diagonal's imaginary part as +0.  `scratch` = at least the fp64 words
 * inr_coil_gram_scratch gives for (C, N) -- a function of its arguments alone; `scratch_doubles` is what the caller's
 * buffer holds.  A workgroup takes INR_COIL_TILE_PIXELS pixels of all C coils per step, with 16-byte loads when `data`
 * is 16-byte aligned and N is even (else 8-byte loads).  Two launches on `stream`; nothing is allocated, nothing is read
 * back, capturable in a graph.  inr_mi355x/coils.py::coil_gram_numpy restates it in numpy.
 * inr_coil_apply: out [M][N][2] = A [M][K][2] (device, row-major complex fp32) times in [K][N][2]:
 * y_m[p] = sum_k A[m][k] x_k[p] in fp32, k = 0..K-1 in order (re += ar xr - ai xi, im += ar xi + ai xr).  Compression
 * passes the K x C matrix, expansion back to physical coils its conjugate transpose.  One launch; 16-byte loads and
 * stores when in / out are 16-byte aligned and N is even.  coils.py::coil_apply_numpy restates it.
 * INR_ERR_INVALID before any launch: a null pointer; C, M or K outside 1..INR_COIL_MAX; N < 1 or N >= 2^31; data / in /
 * out not 8-byte aligned; scratch_doubles short of the query; out overlapping in or A. */
#define INR_COIL_MAX 32
#define INR_COIL_TILE_PIXELS 128
int inr_coil_gram_scratch(int32_t C, int64_t N, int64_t* scratch_doubles);
int inr_coil_gram(const float* data, int32_t C, int64_t N, double* gram, double* scratch, int64_t scratch_doubles,
                  void* stream);
int inr_coil_apply(const float* in, const float* A, int32_t M, int32_t K, int64_t N, float* out, void* stream);

/* (v7 addition) Off-grid samples of the continuous k-space of coil images (no reference counterpart; DESIGN.md section
 * 4.19).  img [C][H][W][2]: complex fp32 coil images, centred as an inverse centred FFT leaves them; pos [M][2]: fp64
 * (u_y, u_x) in index units, any finite value (the transform is periodic); out [C][M][2] fp32,
 *   out[c][m] = 1/sqrt(H W) sum_y sum_x img[c][y][x] exp(-2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
 * c_y = H/2, c_x = W/2 (integer division): at integer positions the centred FFT of the image.  The phase is reduced in
 * fp64 (its fractional part is taken before the multiplication by 2 pi), phasors and sums are fp32, the order of the
 * sums is fixed (no atomics): two calls give the same bits.  `scratch` (device, 16-byte aligned) holds at least what
 * inr_nudft_scratch gives for (C, H, W, M) -- a function of its arguments alone (the phasor tables: 2 (W' + H') M' floats
 * with W' = W rounded up to 16, H' to 64 and M' = M to INR_NUDFT_TILE); `scratch_floats` is what the caller's buffer
 * holds.  Two launches on `stream`, nothing allocated, nothing read back.
 * inr_mi355x/trajectory.py::nudft_numpy restates it in fp64.
 * INR_ERR_INVALID before any launch: a null pointer; C outside 1..INR_COIL_MAX; H or W < 1; H * W >= 2^31; M < 1 or
 * M >= 2^31; img / pos / out not 8-byte or scratch not 16-byte aligned; scratch short of the query; out overlapping img
 * or pos; scratch overlapping any of them. */
#define INR_NUDFT_TILE 64
int inr_nudft_scratch(int32_t C, int64_t H, int64_t W, int64_t M, int64_t* scratch_floats);
int inr_nudft(const float* img, int32_t C, int64_t H, int64_t W, const double* pos, int64_t M, float* out,
              float* scratch, int64_t scratch_floats, void* stream);

/* (v7 addition) The conjugate transpose of inr_nudft: off-grid k-space samples back onto the image grid (no reference
 * counterpart).  val [C][M][2]: complex fp32 samples; pos [M][2]: fp64 (u_y, u_x) as for
 * inr_nudft; w [M]: fp32 weights (a density compensation), or null for all ones; out [C][H][W][2] fp32,
 *   out[c][y][x] = 1/sqrt(H W) sum_m w[m] val[c][m] exp(+2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
 * c_y = H/2, c_x = W/2: with every integer grid point as a position and w null, the inverse centred FFT.  It reads the
 * phasor tables inr_nudft reads (fp64 phase reduction, fp32 entries), so the two calls are transposes of each other up
 * to the rounding of their fp32 sums; the order of the sums is fixed (no atomics): two calls give the same bits.
 * `scratch` (device, 16-byte aligned) holds at least what inr_adjoint_nudft_scratch gives for (C, H, W, M): 2 (W' + H') M'
 * floats with W' and H' rounded up to 64 and M' = M to 64.  Two launches on `stream`, nothing allocated, nothing read
 * back.  inr_mi355x/trajectory.py::nudft_adjoint_numpy restates it in fp64.
 * INR_ERR_INVALID before any launch: a null pointer other than w; C outside 1..INR_COIL_MAX; H or W < 1 or > 2^31 - 64;
 * H * W >= 2^31; M < 1 or M >= 2^31; val / pos / out not 8-byte, w not 4-byte or scratch not 16-byte aligned; scratch
 * short of the query; out overlapping val, pos or w; scratch overlapping any of them. */
int inr_adjoint_nudft_scratch(int32_t C, int64_t H, int64_t W, int64_t M, int64_t* scratch_floats);
int inr_adjoint_nudft(const float* val, const double* pos, const float* w, int32_t C, int64_t H, int64_t W, int64_t M,
                      float* out, float* scratch, int64_t scratch_floats, void* stream);

/* (v7 addition) Table-based (Kaiser-Bessel) gridding: inr_nudft and inr_adjoint_nudft approximated in O(M J^2) device work
 * around an FFT of the twice oversampled grid that the CALLER runs between the calls -- the library does not link an FFT
 * (no reference counterpart).  Fixed parameters: Gy = 2 H, Gx = 2 W; J = INR_NUFFT_TAPS = 6 taps
 * per axis; kb(t) = I0(beta sqrt(1 - (2 t / J)^2)) / I0(beta) on |t| <= J / 2, beta = pi sqrt((J / 2)^2 (3 / 2)^2 - 0.8).
 * A sample at pos = (u_y, u_x) sits at g = 2 (u - c) + G / 2 per axis (c = n / 2, integer division; fp64, reduced into
 * [0, G): the operators are periodic in u); its taps are the cells j0 .. j0 + 5, j0 = ceil(g - 3), modulo G, with
 * weights kb(g - j) evaluated in fp64 and stored as fp32.  apod_y [H], apod_x [W] (device, fp32): the apodisation
 * a(nu) = J sinh(s) / (s I0(beta)), s = sqrt(beta^2 - (pi J nu)^2), at nu = (y - c) / G, evaluated by the caller in fp64.
 *
 *   forward, the approximation of inr_nudft:
 *     inr_nufft_prepare  img [C][H][W][2] -> grid [C][Gy][Gx][2]: img[c][y][x] * 2 / (apod_y[y] apod_x[x]) at
 *                        (y - c_y + H, x - c_x + W), zero elsewhere; every element of grid is written
 *     (caller)           the centred orthonormal FFT of every [Gy][Gx] plane
 *     inr_nufft_interp   grid, pos [M][2] -> out [C][M][2]: the 36 taps of every sample, summed in the order ky, kx
 *   adjoint with weights, the approximation of inr_adjoint_nudft:
 *     inr_nufft_spread   val [C][M][2], pos, w [M] or null -> grid: grid[c][j] = sum over the samples with a tap on cell j
 *                        of kb_y kb_x w[m] val[c][m]; a gather over a cell list, no atomics; every element is written
 *     (caller)           the centred orthonormal inverse FFT of every plane
 *     inr_nufft_finish   grid -> out [C][H][W][2]: the centre H x W times 2 / (apod_y[y] apod_x[x])
 * In exact arithmetic the two chains are conjugate transposes of each other (the 2 is sqrt(Gy Gx) / sqrt(H W)).  Sums have
 * a fixed order: two calls give the same bits.
 * The cell list of inr_nufft_spread: bins of INR_NUFFT_TILE x INR_NUFFT_TILE grid cells, T = ceil(Gy / 16) ceil(Gx / 16)
 * of them, bin (floor(g_y) / 16) * ceil(Gx / 16) + floor(g_x) / 16 for a sample; order [M] (int32): the sample indices
 * sorted by bin, ascending within a bin; bin_start [T + 1] (int32): bin b is order[bin_start[b] .. bin_start[b + 1]).
 * inr_mi355x/trajectory.py::nufft_bins builds them.  Both are device-readable and TRUSTED: where they are host-visible
 * (pinned host memory) bin_start is checked -- bin_start[0] = 0, non-decreasing, bin_start[T] = M -- and refused with
 * INR_ERR_INVALID; otherwise the kernel clamps what it reads of them (entries of bin_start into [0, M]; an order[] entry
 * outside [0, M) adds zeros), so that malformed arrays lose samples but read nothing out of bounds.
 * `scratch` (device, 16-byte aligned; interp and spread) holds at least what inr_nufft_scratch gives for (C, H, W, M):
 * 14 M' floats, M' = M rounded up to 64 -- the taps, which every call writes anew, once for all coils.
 * prepare, finish: one launch; interp, spread: two.  All on `stream`, nothing allocated, nothing read back.
 * inr_mi355x/trajectory.py::nufft_numpy / nufft_adjoint_numpy restate the two chains in fp64.
 * INR_ERR_INVALID before any launch: a null pointer other than w; C outside 1..INR_COIL_MAX; H or W < 3 (six taps must
 * land on six cells); H * W >= 2^31; M < 1 or M >= 2^31; img / val / pos / out not 8-byte, grid or scratch not 16-byte,
 * w / apod_y / apod_x / bin_start / order not 4-byte aligned; scratch short of the query; an output (grid, out) that
 * overlaps an input of the same call; scratch overlapping any of the call's arrays; a host-visible bin_start that fails
 * the check above. */
#define INR_NUFFT_TAPS 6
#define INR_NUFFT_TILE 16
int inr_nufft_scratch(int32_t C, int64_t H, int64_t W, int64_t M, int64_t* scratch_floats);
int inr_nufft_prepare(const float* img, const float* apod_y, const float* apod_x, int32_t C, int64_t H, int64_t W,
                      float* grid, void* stream);
int inr_nufft_interp(const float* grid, const double* pos, int32_t C, int64_t H, int64_t W, int64_t M, float* out,
                     float* scratch, int64_t scratch_floats, void* stream);
int inr_nufft_spread(const float* val, const double* pos, const float* w, const int32_t* bin_start, const int32_t* order,
                     int32_t C, int64_t H, int64_t W, int64_t M, float* grid, float* scratch, int64_t scratch_floats,
                     void* stream);
int inr_nufft_finish(const float* grid, const float* apod_y, const float* apod_x, int32_t C, int64_t H, int64_t W,
                     float* out, void* stream);

/* (v7 addition) Off-grid SENSE fits on calibrated coil maps (no reference counterpart): the
 * gridding operators above with the coil product of inr_sense_apply / inr_sense_adjoint fused into their first and last
 * pass, on a grid in PLAIN layout -- the layout a plain (unshifted) 2-D FFT reads and writes.  Gy = 2 H and Gx = 2 W are
 * even, so fftshift and ifftshift are both the roll by (H, W): the plain grid is the centred grid of inr_nufft_* rolled
 * by (H, W), cell (jy, jx) of the centred grid lives at ((jy + H) mod Gy, (jx + W) mod Gx), and pixel (y, x) at
 * ((y - H/2) mod Gy, (x - W/2) mod Gx) with integer H/2, W/2.  The caller's FFT between the calls is the plain
 * orthonormal one; no shifted copy and no coil images are made.
 *   inr_nufft_interp_plain, inr_nufft_spread_plain: inr_nufft_interp / inr_nufft_spread on a plain-layout grid -- same
 *       arguments, checks, scratch, bins and cell list, same arithmetic in the same order (interp's output is bit for bit
 *       that of inr_nufft_interp on the centred grid; spread's grid is bit for bit the roll of inr_nufft_spread's).
 *   inr_sense_nufft_prepare: img [H*W,2], maps [G,H*W,2] -> grid [G,Gy,Gx,2].  Per coil and pixel, in fp32, nothing
 *       contracted: (xr, xi) = inr_sense_apply's x (re = sr*ir - si*ii; im = sr*ii + si*ir; scale*re, scale*im), then
 *       d = 2 / (apod_y[y] * apod_x[x]) and the cell (xr * d, xi * d).  Padding cells are written as zeros: every
 *       element of grid is written.  Bit for bit inr_sense_apply(shift 0) + inr_nufft_prepare, rolled by (H, W).
 *   inr_sense_nufft_finish: grid, maps -> dimg [H*W,2].  Per pixel, coils in ascending order from zero:
 *       (gr, gi) = the pixel's cell; v = (gr * d, gi * d); ur = scale*vr; ui = scale*vi;
 *       t_g = (sr*ur + si*ui, sr*ui - si*ur); dI = (((0 + t_0) + t_1) + ...) + t_{G-1};
 *       dimg[p] = dI, or with accumulate = 1 dimg[p] + dI (one fp32 addition).  Bit for bit inr_nufft_finish of the grid
 *       rolled back + inr_sense_adjoint(shift 0).  One lane owns a pixel for every coil: no atomics, same bits every call.
 * prepare / finish: one launch on `stream`; with every pointer 16-byte aligned and W and W/2 even two neighbouring cells
 * move per 16-byte access, else one per 8-byte access; the results do not depend on which path ran.
 * INR_ERR_INVALID before any launch: a null pointer; G outside 1..INR_COIL_MAX; H or W < 3; H * W >= 2^31; a non-finite
 * scale; accumulate outside {0, 1}; img / dimg / maps / grid not 8-byte or apod_y / apod_x not 4-byte aligned; the output
 * (grid, dimg) overlapping an input.  The _plain entries refuse what inr_nufft_interp / inr_nufft_spread refuse. */
int inr_nufft_interp_plain(const float* grid, const double* pos, int32_t C, int64_t H, int64_t W, int64_t M, float* out,
                           float* scratch, int64_t scratch_floats, void* stream);
int inr_nufft_spread_plain(const float* val, const double* pos, const float* w, const int32_t* bin_start,
                           const int32_t* order, int32_t C, int64_t H, int64_t W, int64_t M, float* grid, float* scratch,
                           int64_t scratch_floats, void* stream);
int inr_sense_nufft_prepare(const float* img, const float* maps, const float* apod_y, const float* apod_x, int32_t G,
                            int64_t H, int64_t W, float scale, float* grid, void* stream);
int inr_sense_nufft_finish(const float* grid, const float* maps, const float* apod_y, const float* apod_x, int32_t G,
                           int64_t H, int64_t W, float scale, float* dimg, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INR_ABI_H */
