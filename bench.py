#!/usr/bin/env python3
"""bench.py -- coord-samples/sec (fwd+bwd) fitting synthetic 640x368x15-coil k-space.

Workload (BASELINE.json configs[1]): SIREN depth 5 / width 256 / gauss-512 input, last_tanh,
k-space, normalization 'coil', L2, lr 3e-5, batch 25 000 coordinates per GPU.  One "step" =
fused encode->forward->loss->backward kernel + slab reduction (+ RCCL all-reduce of the 1.3 MB
gradient when N>1) + Adam/re-pack kernel, on sequential batches resident in HBM.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0.  Data is synthetic (seeded phantom), weights are random-init.  A plain run sets up, warms
up, times the K steps and prints the headline; --full adds the roofline and per-kernel timings, the PSNR read-out, the CPU
baseline, batch 65 536, the bf16 path, config 5 and config 4.  --dump-outputs writes what the last timed step left to
its caller (loss, parameters, gradient, Adam moments) as DIR/<name>.npy, before anything of --full runs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FLOP_PER_SAMPLE = 1_707_008  # SIREN 5x256/in512 fwd + dW + dX, 2 FLOP per MAC
# the fp32 path splits them over two kernels: the fused kernel (forward, loss, dX, the 2-row last layer's dW) and the
# batch-level GEMM for dW of the four 256-row layers (inr_dw_gemm.hip)
FLOP_DW_GEMM = 2 * (512 * 256 + 3 * 256 * 256)
FLOP_FUSED_F32 = FLOP_PER_SAMPLE - FLOP_DW_GEMM
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md chip table: v_mfma_f32_32x32x2_f32 dense peak

CONFIG = {
    "model": "SIREN", "loss": "L2", "optimizer": "Adam", "lr": 3e-5, "beta1": 0.9, "beta2": 0.999,
    "weight_decay": 0.0, "max_epoch": 1000, "batch_size": 25000, "transform": False, "normalization": "coil",
    "net": {"network_input_size": 512, "network_output_size": 2, "network_depth": 5, "network_width": 256,
            "last_tanh": True},
    "encoder": {"embedding": "gauss", "scale": 4, "embedding_size": 256, "coordinates_size": 3},
}
SHAPE = (15, 640, 368)


def psnr_read_steps(total: int, spe: int, bs: int, coil_rows: int, n_coils: int):
    """Step counts at which the fit's PSNR is read (models/utils.py:236-250 evaluates the whole k-space; the reference reads
    it every val_epoch epochs, train.py:199-231).  A single read of this loop is spiky: batches walk through the coils in
    order and a read right behind a coil's k-space centre can sit decibels low for a few hundred steps in EITHER precision
    (profiles/r03_psnr_trajectory.txt).  The smooth statistic: the mean over the last full epoch's end-of-coil reads -- the
    step after which coil c has been swept, c = 0 .. n_coils-1, the last of them the epoch's end -- which samples every phase
    of the sweep once.  Returned: those n_coils steps, the epoch boundary before them, and `total` itself."""
    e1 = (total // spe) * spe          # end of the last full epoch
    e0 = e1 - spe                      # ... and its start (= the boundary before)
    if e0 < 0:
        return [total], []
    coil = [e0 + min(spe, -(-((c + 1) * coil_rows) // bs)) for c in range(n_coils)]
    return sorted(set([e0] * (e0 > 0) + coil + [total])), coil


def fit_with_reads(tr, start: int, total: int, reads):
    """steps start .. total-1 of the trainer's loop, its PSNR read after every step count in `reads`"""
    spe, out = tr.steps_per_epoch, {}
    for s_ in range(start, total):
        tr.step(s_ // spe, s_ % spe)
        if s_ + 1 in reads:
            out[s_ + 1] = tr.evaluate()
    return out


def psnr_summary(reads: dict, coil_steps, ref_reads: dict = None):
    """mean / spread over the end-of-coil reads; with `ref_reads` (same steps) also the paired differences"""
    import statistics as st
    vals = [reads[k] for k in coil_steps if k in reads]
    out = {"reads_db": {str(k): reads[k] for k in sorted(reads)}, "coil_end_steps": list(coil_steps)}
    if len(vals) >= 2:
        out["mean_db"], out["std_db"], out["min_db"], out["max_db"] = st.mean(vals), st.pstdev(vals), min(vals), max(vals)
    if ref_reads is not None:
        d = [reads[k] - ref_reads[k] for k in coil_steps if k in reads and k in ref_reads]
        if len(d) >= 2:
            out["vs_reference"] = {"delta_of_means_db": st.mean(d), "std_of_deltas_db": st.pstdev(d),
                                   "max_abs_delta_db": max(abs(x) for x in d), "n_reads": len(d),
                                   "within_0p1_db": abs(st.mean(d)) <= 0.1}
    return out


def usable_cores() -> int:
    """Host threads this job may actually use: affinity mask, cgroup quota, and the GPU box's
    per-GPU CPU share (16) -- oversubscribing 256 visible cores made the first baseline 40x slower."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return int(os.environ.get("INR_CPU_THREADS", min(n, 16)))


def cpu_baseline(image, coords, shape, seconds=15.0, psnr_steps=1000, read_steps=()):
    """The oracle (CPU restatement of the reference's loop train.py:155-231: encode -> SIREN -> 0.5*MSE -> autograd
    -> Adam, per-epoch LambdaLR, sequential batches) on this host's cores.  One run serves two purposes: its first
    `seconds` of steps (after two warm-up steps) are the timed cpu_baseline sample, and when `psnr_steps` > 0 it keeps
    going to that step count and is evaluated (models/utils.py:236-250) -- the reference-side PSNR the HIP paths are
    held to (north-star: within 0.1 dB).  The oracle is the checker here, never the thing shipped."""
    import oracle as O
    torch.set_num_threads(usable_cores())
    cfg = dict(CONFIG)
    torch.manual_seed(0)
    B = O.encoder_init(cfg["encoder"])
    sd = O.init_model("SIREN", cfg["net"])
    bs = cfg["batch_size"]
    stamps = []
    snaps = {}  # the oracle's weights at the PSNR read steps (1.3 MB each)

    def rec(step, sd_, loss):
        stamps.append(time.perf_counter())
        if step in read_steps:
            snaps[step] = {k_: v.detach().clone() for k_, v in sd_.items()}

    class _Enough(Exception):
        pass

    def rec_timed(step, sd_, loss):
        rec(step, sd_, loss)
        if len(stamps) >= 5 and stamps[-1] - stamps[2] >= seconds:
            raise _Enough

    n_steps = psnr_steps if psnr_steps > 0 else 10 ** 9
    try:
        O.train_single_scale(cfg, sd, B, coords, image, n_steps, record=rec if psnr_steps > 0 else rec_timed)
    except _Enough:
        pass
    # timed sample: steps 3 .. k (whole 25 000-row batches: the first epoch's, none of them the short last batch)
    k = len(stamps) - 1
    for i in range(3, len(stamps)):
        if stamps[i] - stamps[2] >= seconds or i >= 140:  # stamps[140] = step 141, the last full batch of epoch 0
            k = i
            break
    dt = stamps[k] - stamps[2]
    out = {"value": (k - 2) * bs / dt, "unit": "coord-samples/s", "cores": torch.get_num_threads(), "kind": "port",
           "sample": f"{k - 2} steps x {bs} rows of the same workload (oracle: PyTorch-CPU fp32, "
                     f"encode+fwd+0.5*MSE+autograd+Adam), {dt:.1f} s"}
    # the same step fed the reference's way: batches collated item by item by a torch DataLoader
    # over the per-coordinate dataset -- the host-bound figure the reference's loop would see on these cores.  Four batches.
    loader = torch.utils.data.DataLoader(O.PerItemDataset(coords, image), batch_size=bs, shuffle=False, num_workers=0)
    sd2 = {k_: v.clone().requires_grad_(True) for k_, v in sd.items()}
    opt_state = O.adam_init(sd2)
    t_data = t_all = 0.0
    it = iter(loader)
    for i in range(5):
        ta = time.perf_counter()
        xb, gb, _, _ = next(it)
        tb = time.perf_counter()
        loss = O.loss_l2_half(O.siren_forward(sd2, O.encode(xb, B, "gauss"), cfg["net"]), gb)
        grads = dict(zip(sd2.keys(), torch.autograd.grad(loss, list(sd2.values()))))
        with torch.no_grad():
            O.adam_step(sd2, grads, opt_state, cfg["lr"], 0.9, 0.999, 1e-8, 0.0)
        tc = time.perf_counter()
        if i > 0:  # (the first batch pays the iterator's start-up)
            t_data += tb - ta
            t_all += tc - ta
    out["dataloader_bound"] = {"value": 4 * bs / t_all, "unit": "coord-samples/s", "data_only": 4 * bs / t_data,
                               "sample": f"4 batches x {bs} rows through a per-item DataLoader (default collate, no workers) "
                                         f"+ the same CPU step: {t_all / 4 * 1e3:.0f} ms per batch, {t_data / 4 * 1e3:.0f} ms "
                                         "of it collating"}
    if psnr_steps > 0:
        with torch.no_grad():
            pred = torch.cat([O.model_forward("SIREN", sd, O.encode(coords[lo:lo + (1 << 18)], B, "gauss"), cfg["net"])
                              for lo in range(0, coords.shape[0], 1 << 18)], 0)
        out["reference_psnr"] = {"steps": len(stamps), "seconds": stamps[-1] - stamps[0],
                                 "psnr_db": float(O.psnr(O.reconstruct(image, shape, False),
                                                         O.reconstruct(pred, shape, False)))}
    out["_snapshots"] = snaps  # (popped by main: not part of the JSON line)
    return out


BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md chip table: dense bf16 MFMA


def bf16_path(cfg, image, coords, shape, dev, args, fused_kernel_ms_of, main_line):
    """The same workload on the bf16-MFMA throughput path (config key precision: bf16; fp32 master weights and
    Adam).  Reported next to the graded fp32 line, never instead of it: bf16 operands cannot meet the 1e-5 parity
    bar, so this object carries its own PSNR after the same number of steps (north-star: within 0.1 dB)."""
    from inr_mi355x.train import INRTrainer
    tr = INRTrainer(dict(cfg, precision="bf16"), image, coords, shape, dev, seed=0, graph_steps=bool(args.graph))
    spe = tr.steps_per_epoch

    def run(n, start):
        for i in range(n):
            tr.step((start + i) // spe, (start + i) % spe)

    tr.prepare_graphs()
    run(args.warmup, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps, args.warmup)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rows = 0
    for i in range(args.steps):
        it = (args.warmup + i) % spe
        rows += min((it + 1) * tr.bs, tr.n) - it * tr.bs
    def path_ms(batch, reps=50):
        """fused kernel + bf16 weight-gradient GEMM + slab reduction (inr_train_step with grads), no Adam"""
        x, gt = tr.coords[:batch], tr.image[:batch]
        for _ in range(5):
            tr.engine.train_step(x, tr.enc_B, gt, tr.loss)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            tr.engine.train_step(x, tr.enc_B, gt, tr.loss)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    k_ms = fused_kernel_ms_of(tr, args.batch)
    p_ms = path_ms(args.batch)
    ach = FLOP_PER_SAMPLE * args.batch / (p_ms * 1e-3) / 1e12
    # the roofline fraction is quoted on the whole gradient path (all 1 707 008 FLOP per coordinate happen in it):
    # fused kernel (encoder, forward, loss, dX) + dw_gemm_bf16_kernel (dW, db) + slab reduction
    res = {"dtype": "bf16", "value": rows / dt, "unit": "coord-samples/s", "ms_per_step": dt / args.steps * 1e3,
           "kernels": "inr_siren_bf16_kernel + dw_gemm_bf16_kernel + reduce_slabs_real_kernel",
           "fused_kernel_ms": k_ms, "gradient_path_ms": p_ms, "achieved": ach,
           "peak": BF16_MFMA_PEAK_TFLOPS, "frac": ach / BF16_MFMA_PEAK_TFLOPS, "roofline_unit": "TFLOP/s",
           "speedup_vs_f32_step": (rows / dt) / main_line["value"]}
    done = args.warmup + args.steps
    if args.psnr_steps and args.psnr_steps > done:
        reads, coil_steps = psnr_read_steps(args.psnr_steps, spe, tr.bs, SHAPE[1] * SHAPE[2], SHAPE[0])
        reads = [r for r in reads if r > done]
        coil_steps = [r for r in coil_steps if r > done]
        b_reads = fit_with_reads(tr, done, args.psnr_steps, set(reads))
        res["psnr_at_1k_steps"] = {"steps": args.psnr_steps, "psnr_db": b_reads[args.psnr_steps]}
        # the smooth criterion: mean over the last full epoch's end-of-coil reads against the reference run's (north star:
        # within 0.1 dB), with the spread of the paired differences
        res["psnr_at_1k_steps"]["last_epoch"] = psnr_summary(b_reads, coil_steps, main_line.get("_ref_reads"))
        st_ = tr.engine.grad_scale_state()
        res["grad_scale_counters"] = {"clipped_steps": st_[8], "flushed_steps": st_[9], "steps": args.psnr_steps}
        if "psnr_at_1k_steps" in main_line:
            res["psnr_at_1k_steps"]["delta_vs_f32_db"] = (res["psnr_at_1k_steps"]["psnr_db"]
                                                          - main_line["psnr_at_1k_steps"]["psnr_db"])
    for _ in range(300):  # (the evaluation sweep and host work above left the GPU idle: warm up before timing)
        tr.engine.train_step(tr.coords[:65536], tr.enc_B, tr.image[:65536], tr.loss)
    ms65, p65 = fused_kernel_ms_of(tr, 65536), path_ms(65536)
    a65 = FLOP_PER_SAMPLE * 65536 / (p65 * 1e-3) / 1e12
    res["batch_65536"] = {"fused_kernel_ms": ms65, "gradient_path_ms": p65, "achieved": a65,
                          "frac": a65 / BF16_MFMA_PEAK_TFLOPS, "coord_samples_per_s": 65536 / (p65 * 1e-3)}
    return res


def config5_percoil(dev, steps=15, warmup=4):
    """BASELINE config 5 -- radial acc-4 undersampling, per-coil batches (one 640 x 368 coil = 235 520 coordinates per
    step, the forward pass on all of them, the loss on the ~59 k sampled ones), TV on the coil's grid (train.py:158-192
    with per_coil / use_tv; losses.py:326-343), SIREN 5x256 -- on both precisions.  The step is split at the loss (forward
    with stash -> loss + TV gradient -> backward + weight-gradient GEMM -> Adam).  Algorithmic FLOP per coordinate as the
    graded workload's (every row goes through forward, dX and dW: unsampled rows carry a zero pointwise gradient but
    their TV gradient)."""
    import yaml
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_radial_tv_bf16.yaml")))
    image, coords, shape = make_kspace(2, SHAPE[1], SHAPE[2], seed=1234, normalization="coil")
    out = {"workload": "SIREN 5x256 gauss-512, radial-4 mask, per-coil batches of 640x368 = 235 520 coordinates, L2 + TV "
                       "(split step: forward | loss + TV | backward + dW GEMM | Adam)", "rows_per_step": SHAPE[1] * SHAPE[2]}
    for prec in ("f32", "bf16"):
        c = dict(cfg)
        c.pop("precision")
        if prec == "bf16":
            c["precision"] = "bf16"
        tr = INRTrainer(c, image, coords, shape, dev, seed=0, mask_seed=7)
        spe = tr.steps_per_epoch
        for i in range(warmup):
            tr.step(0, i % spe)
        # wall clock over `steps` steps, best round: a step is ~10 launches for 0.6-4 ms of GPU work, and in a freshly started
        # process the host side of the first rounds has measured 10-60x that (first seconds of a box; kernel durations under
        # rocprofv3 are normal from the first launch on).  Rounds repeat until two in a row agree within 10 %, at most 8.
        rounds = []
        for rep in range(8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                tr.step(0, (warmup + i) % spe)
            torch.cuda.synchronize()
            rounds.append((time.perf_counter() - t0) / steps * 1e3)
            if rep >= 2 and abs(rounds[-1] - rounds[-2]) < 0.1 * rounds[-1]:
                break
        ms = sorted(rounds)[len(rounds) // 2]  # the median round is the headline; the best one is reported beside it
        peak = BF16_MFMA_PEAK_TFLOPS if prec == "bf16" else F32_MFMA_PEAK_TFLOPS
        ach = FLOP_PER_SAMPLE * tr.bs / (ms * 1e-3) / 1e12
        out[prec] = {"ms_per_step": ms, "coord_samples_per_s": tr.bs / (ms * 1e-3), "achieved_tflops": ach, "peak": peak,
                     "frac": ach / peak, "sampled_fraction": float(tr.mask_cpu.float().mean()),
                     "ms_per_step_best_round": min(rounds), "rounds_ms": rounds}
        del tr
    out["bf16_speedup"] = out["f32"]["ms_per_step"] / out["bf16"]["ms_per_step"]
    return out


MS_FLOP_PER_SAMPLE = 19_423_232  # MultiscaleKFourier 8x512/in512, 4 heads, live layers only
MS_CONFIG = {
    "model": "MultiscaleKFourier", "loss": "LSL", "loss_opts": {"hdr_eps": 3e-3, "hdr_ff_sigma": 2, "hdr_ff_factor": 0.5},
    "optimizer": "Adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "weight_decay": 0.0, "max_epoch": 2000,
    "batch_size": 100000, "normalization": "max", "partition": {"no_steps": 40, "no_models": 4},
    "net": {"network_input_size": 512, "network_output_size": 2, "network_depth": 8, "network_width": 512},
    "encoder": {"embedding": "gauss", "scale": 4, "embedding_size": 256, "coordinates_size": 3},
}


def config4_shard_sweep(tr, dev, reps=6):
    """ONE GPU, the step a rank of an N-GPU job would run: the gradient path on 100 000 / N rows of batch 0 (global count
    and consistency counts kept: exactly what rank 0 computes) and the Adam update, timed apart with HIP events.  From
    them the ceiling of the strong-scaling curve,  T(1) / (T_grad(N) + T_adam + all-reduce estimate),  with the all-reduce
    of the flat gradient priced as a ring over xGMI links at 100 GB/s effective:  2 (N - 1) / N x bytes / (rings x 100 GB/s)
    for ONE ring and for FOUR (RCCL builds several rings over the 7 links; the measured value comes from SCALE runs).
    No curve is claimed from this: it says where the time of a shard-sized step goes before a multi-GPU box is there."""
    eng = tr.engine
    lo, hi = 0, min(tr.bs, tr.n)
    cons = tr._cons_spec(0, lo, hi)
    lr = tr.config["lr"]
    out = {"rows_global": hi - lo, "allreduce_bytes": 4 * (eng.n_params + 1), "by_n": {}}

    def timed(fn, n):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    t_adam = timed(lambda: eng.adam_step(lr, tr.config["beta1"], tr.config["beta2"], 1e-8, tr.config["weight_decay"]), reps)

    def sharded_local(n):
        """what MLPEngine.adam_step_sharded launches on a rank of n besides the two collectives: Adam on P / n entries, the
        chunk copies, the copy back of the gathered vector and the re-pack"""
        from inr_mi355x import _lib as L
        from inr_mi355x.engine import _ptr
        P = eng.n_params
        chunk = -(-(P + 1) // n)
        gchunk, pchunk, pgather = (torch.zeros(chunk, device=dev), torch.zeros(chunk, device=dev),
                                   torch.zeros(chunk * n, device=dev))
        pgather[:P].copy_(eng.params)
        hi_ = min(chunk, P)

        def fn():
            eng.step += 1
            L.check(eng.lib.inr_adam_step_shard(eng.plan, _ptr(eng.params, "params"), _ptr(gchunk, "g"),
                                                _ptr(eng.exp_avg, "m"), _ptr(eng.exp_avg_sq, "v"), 0, hi_, lr,
                                                tr.config["beta1"], tr.config["beta2"], 1e-8, tr.config["weight_decay"],
                                                0.0, 0.0, eng.step, eng._stream()))
            pchunk.copy_(gchunk)
            pchunk[:hi_].copy_(eng.params[:hi_])
            eng.params.copy_(pgather[:P])
            eng.pack()
        return timed(fn, reps)

    t1 = None
    for n in (1, 2, 4, 8):
        shi = lo + (hi - lo) // n
        x, g, d = tr._inputs(lo, shi), tr.image[lo:shi], tr.dist[lo:shi]
        t_grad = timed(lambda: eng.train_step(x, tr.enc_B, g, tr.loss, count=hi - lo, dist=d, scale=tr.scale, cons=cons), reps)
        nt, nb = eng.launch_dims(shi - lo)
        if n == 1:
            t1 = t_grad + t_adam
        ar = [2.0 * (n - 1) / n * out["allreduce_bytes"] / (rings * 100e9) * 1e3 for rings in (1, 4)]
        t_sh = sharded_local(n) if n > 1 else t_adam
        out["by_n"][str(n)] = {"rows": shi - lo, "tiles": nt, "workgroups": nb, "grad_path_ms": t_grad, "adam_ms": t_adam,
                               "sharded_update_ms": t_sh,
                               "allreduce_est_ms": {"one_ring": ar[0], "four_rings": ar[1]},
                               "ceiling": {"one_ring": t1 / (t_grad + t_adam + ar[0]),
                                           "four_rings": t1 / (t_grad + t_adam + ar[1])},
                               # reduce-scatter + all-gather move the bytes of one ring all-reduce
                               "ceiling_sharded_update": {"one_ring": t1 / (t_grad + t_sh + ar[0]),
                                                          "four_rings": t1 / (t_grad + t_sh + ar[1])}}
    return out


def multiscale_config4(dev, rank, world, pg, steps, warmup, barrier):
    """BASELINE config 4 -- the workload the north star's 1 -> 8 GPU scaling target names: MultiscaleKFourier 8x512,
    LSL + 0.1 consistency, k-means ring partition, GLOBAL batch 100 000 sharded over the ranks (strong scaling),
    one SUM all-reduce of the 17.9 MB gradient per step (train_kspace_multiscale.py:161-201)."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    image, coords, shape = make_kspace(*SHAPE, seed=1234, normalization="max")
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    tr = MultiscaleTrainer(dict(MS_CONFIG), image, coords, dist, None, shape, dev, seed=0, rank=rank, world=world,
                           process_group=pg)
    spe = tr.steps_per_epoch

    def run(n, start):
        for i in range(n):
            tr.step((start + i) // spe, (start + i) % spe)

    run(warmup, 0)
    barrier()
    t0 = time.perf_counter()
    run(steps, warmup)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist_
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist_.all_reduce(t, op=dist_.ReduceOp.MAX)
        dt = float(t)
    rows = 0
    for i in range(steps):
        it = (warmup + i) % spe
        rows += min((it + 1) * tr.bs, tr.n) - it * tr.bs
    ach = MS_FLOP_PER_SAMPLE * rows / dt / 1e12
    sweep = config4_shard_sweep(tr, dev) if world == 1 else None
    return {"shard_sweep": sweep,
            "workload": "MultiscaleKFourier 8x512 gauss-512, LSL + 0.1 consistency, 4-ring k-means partition, "
                        "synthetic 640x368x15-coil", "value": rows / dt, "unit": "coord-samples/s", "n_gpus": world,
            "scaling": "strong", "global_batch": tr.bs, "steps": steps, "warmup": warmup,
            "ms_per_step": dt / steps * 1e3, "radii": [float(r) for r in tr.radii],
            "achieved_tflops_all_gpus": ach, "frac_f32_mfma_per_gpu": ach / world / F32_MFMA_PEAK_TFLOPS,
            "allreduce_bytes": 4 * (tr.engine.n_params + 1),
            "update": "sharded (reduce-scatter, Adam on 1/N, all-gather, re-pack)" if tr.sharded_update else "replicated"}


def dump_outputs(d: str, tr, loss) -> None:
    """What the timed step hands its caller: the loss it returned and the engine state it left (flat parameters,
    gradient, Adam moments), float32, one .npy per array (4 x 1.3 MB for SIREN 5x256)."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    eng = tr.engine
    arrays = {"loss": loss, "params": eng.params, "grads": eng.grads, "exp_avg": eng.exp_avg,
              "exp_avg_sq": eng.exp_avg_sq}
    for name, t in arrays.items():
        np.save(os.path.join(d, name + ".npy"), t.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=25000, help="coordinates per GPU per step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16-MFMA throughput path's extra object")
    ap.add_argument("--psnr-steps", type=int, default=1000, help="total steps before the PSNR read-out (N=1)")
    ap.add_argument("--no-multiscale", action="store_true", help="skip the config-4 (multi-scale) object")
    ap.add_argument("--no-config5", action="store_true", help="skip the config-5 (radial mask, per-coil TV) object")
    ap.add_argument("--ms-steps", type=int, default=10, help="timed steps of the config-4 object")
    ap.add_argument("--prewarm-ms", type=float, default=600.0,
                    help="untimed gradient-only launches (no Adam: weights and step count do not move) for at least this "
                         "long before the W warm-up steps, so that a short timed window does not sit on a ramping box")
    ap.add_argument("--graph", type=int, default=0,
                    help="N=1: replay each batch's step as one captured HIP graph.  Off by default: measured slower "
                         "than eager launches on this stack (profiles/r02g_graph_vs_eager.json)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: roofline and per-kernel timings, PSNR read-out, CPU baseline, batch 65 536, "
                         "bf16 path, config 5 and config 4 objects (the --no-* and --psnr-steps options act on these)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's loss, parameters, gradient and Adam moments as DIR/<name>.npy")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    # INR_BENCH_REHEARSAL=1: every rank on cuda:0 over gloo -- to rehearse the N > 1 code path on a one-GPU box
    # (numbers from such a run mean nothing; the driver's multi-GPU runs use one GPU per rank over nccl = RCCL)
    rehearsal = os.environ.get("INR_BENCH_REHEARSAL", "0") == "1"
    if rehearsal:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    from inr_mi355x import _lib as L
    import ctypes as C

    image, coords, shape = make_kspace(*SHAPE, seed=1234, normalization="coil")
    cfg = dict(CONFIG)
    cfg["batch_size"] = args.batch * world  # weak scaling: every rank keeps `--batch` rows per step
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=0, rank=rank, world=world, process_group=pg,
                    graph_steps=bool(args.graph))
    spe = tr.steps_per_epoch

    def run(n, start):
        for i in range(n):
            s = start + i
            tr.step(s // spe, s % spe)

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    # before the W warm-up steps: gradient-only launches on batch 0 (no Adam: the weights and the step count do not
    # move) so that workspaces exist, code objects are loaded and the clocks are up when the counted steps begin
    # ... for at least `--prewarm-ms` of wall clock: the driver's `--steps 20 --warmup 5` times a 9 ms window, and 35 launches
    # (17 ms of GPU work) in front of it left the first timed steps on a box that was still ramping (round 3: 0.524 ms per
    # step in that window against 0.475 in a 200-step one, same binary).  `step_ms` below shows what the window saw.
    slo, shi = 0, min(tr.bs, tr.n) // world
    t_pw = time.perf_counter()
    n_pw = 0
    while n_pw < 30 or (time.perf_counter() - t_pw) * 1e3 < args.prewarm_ms:
        for _ in range(10):
            tr.engine.train_step(tr.coords[slo:shi], tr.enc_B, tr.image[slo:shi], tr.loss, count=tr.bs)
        n_pw += 10
        torch.cuda.synchronize()
    prewarm_ms = (time.perf_counter() - t_pw) * 1e3
    tr.prepare_graphs()  # no-op unless graph_steps: captures happen here, not inside the timed region
    run(args.warmup, 0)
    # one HIP event in front of every timed step and one behind the last, on the stream the steps are launched on: the
    # per-step device times show a host stall or a slow first step as such (ms_per_step stays wall clock / steps)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        evs[i].record()
        s_ = args.warmup + i
        loss = tr.step(s_ // spe, s_ % spe)
    evs[args.steps].record()
    barrier()
    dt = time.perf_counter() - t0
    step_ev = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)]
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    rows = 0
    for i in range(args.steps):
        it = (args.warmup + i) % spe
        rows += min((it + 1) * tr.bs, tr.n) - it * tr.bs
    value = rows / dt
    if rank == 0 and args.dump_outputs:  # before --full's objects: they launch more steps on the same engine
        dump_outputs(args.dump_outputs, tr, loss)

    out = {
        "metric": "coord-samples/sec (fwd+bwd) fitting 640x368x15-coil k-space; PSNR@1k steps",
        "value": value, "unit": "coord-samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "step_ms": {"min": min(step_ev), "median": sorted(step_ev)[len(step_ev) // 2], "max": max(step_ev),
                    "first": step_ev[0], "event_sum_per_step": sum(step_ev) / len(step_ev),
                    "note": "device time of each timed step between HIP events on the launch stream (rank 0); ms_per_step is "
                            "wall clock / steps over the same window, barrier to barrier",
                    "prewarm_ms": prewarm_ms, "prewarm_launches": n_pw},
        "config": {"workload": "SIREN 5x256 gauss-512 k-space fit, synthetic 640x368x15-coil, L2, Adam",
                   "batch_per_gpu": args.batch, "global_batch": args.batch * world,
                   "parallelism": f"dp{world}" if world > 1 else "single",
                   "launch": "hip-graph per batch" if tr.graph_steps else "eager"},
    }

    # ---- roofline of the dominant kernel (the fused MLP kernel), HIP events on the launch stream
    eng = tr.engine
    st = torch.cuda.current_stream(dev).cuda_stream

    def fused_kernel_ms_of(tr, batch, reps=50):
        eng = tr.engine
        x, gt = tr.coords[:batch], tr.image[:batch]
        ld = eng.loss_desc(tr.loss, batch)
        ws = eng._ws(*eng.workspace(batch))

        def fused_only():
            L.check(eng.lib.inr_train_step(eng.plan, C.byref(ld), eng.params.data_ptr(), eng.packed.data_ptr(),
                                           x.data_ptr(), tr.enc_B.data_ptr(), gt.data_ptr(), None, batch,
                                           C.byref(ws), None, eng._loss.data_ptr(), st))

        for _ in range(5):
            fused_only()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fused_only()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def fused_kernel_ms(batch, reps=50):
        return fused_kernel_ms_of(tr, batch, reps)

    def gradient_path_ms(batch, reps=50):
        """fused kernel + weight-gradient GEMM + slab reduction (inr_train_step with grads), no Adam"""
        x, gt = tr.coords[:batch], tr.image[:batch]

        def go():
            eng.train_step(x, tr.enc_B, gt, tr.loss)

        for _ in range(5):
            go()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            go()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def fused_kernel_name(batch):
        info = L.StepInfo()
        L.check(eng.lib.inr_plan_step_info(eng.plan, batch, C.byref(info)))
        if info.row_split:
            return (f"inr_mlp_rs_kernel<{info.ncb},SIN> ({info.grid} workgroups x {info.rounds} round(s), tiles of "
                    f"{info.hi}/{info.lo} column blocks of 16 coordinates; v_mfma_f32_16x16x4_f32)")
        return f"inr_mlp_kernel<8,GAUSS,SIN,FUSED> ({info.grid} workgroups x {info.rounds} round(s) of 128-coordinate tiles; v_mfma_f32_32x32x2_f32)"

    if args.full:
        k_ms = fused_kernel_ms(args.batch)
        achieved = FLOP_FUSED_F32 * args.batch / (k_ms * 1e-3) / 1e12
        p_ms = gradient_path_ms(args.batch)
        p_ach = FLOP_PER_SAMPLE * args.batch / (p_ms * 1e-3) / 1e12
        # HBM bytes per launch come from separate rocprofv3 --pmc passes (cannot be collected from inside
        # this process); the committed summary applies only to the workload it was measured on.
        traffic = None
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_latest.json")))
            if args.batch == 25000 and tj["kernel"].split("<")[0] == fused_kernel_name(args.batch).split("<")[0]:
                traffic = tj["bytes_per_launch"]  # (only if the summary was taken on the kernel this run launches)
        except (OSError, ValueError, KeyError):
            pass
        out["roofline"] = {"bound": "mfma", "kernel": fused_kernel_name(args.batch), "achieved": achieved,
                           "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / F32_MFMA_PEAK_TFLOPS,
                           "kernel_ms": k_ms, "flop_per_sample": FLOP_FUSED_F32, "traffic": traffic,
                           "traffic_source": "profiles/traffic_latest.json: HBM bytes per launch from separate rocprofv3 "
                                             "--pmc passes of this workload (FETCH_SIZE x 2 + WRITE_SIZE), committed with "
                                             "the round's profiles -- not measured by this run",
                           "note": "exact-fp32 path (fp32-input MFMA); peak = dense f32 MFMA. This kernel: encoder, "
                                   "forward, loss, dX and the last layer's dW; dW of the 256-row layers is dw_gemm_kernel",
                           "gradient_path": {"kernels": "fused kernel + dw_gemm_kernel<128> + reduce_slabs_real_kernel",
                                             "ms": p_ms, "flop_per_sample": FLOP_PER_SAMPLE, "achieved": p_ach,
                                             "frac": p_ach / F32_MFMA_PEAK_TFLOPS}}
    if args.full and world == 1 and rank == 0:
        done = args.warmup + args.steps
        reads, coil_steps = ([], [])
        if args.psnr_steps and args.psnr_steps > done:
            reads, coil_steps = psnr_read_steps(args.psnr_steps, spe, tr.bs, SHAPE[1] * SHAPE[2], SHAPE[0])
            reads = [r for r in reads if r > done]
            coil_steps = [r for r in coil_steps if r > done]
            f32_reads = fit_with_reads(tr, done, args.psnr_steps, set(reads))
            out["psnr_at_1k_steps"] = {"steps": args.psnr_steps, "psnr_db": f32_reads[args.psnr_steps]}
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(image, coords, shape, psnr_steps=args.psnr_steps, read_steps=set(reads))
            snaps = out["cpu_baseline"].pop("_snapshots")
            ref = out["cpu_baseline"].get("reference_psnr")
            if ref is not None and "psnr_at_1k_steps" in out:  # north-star: PSNR within 0.1 dB of the reference
                out["psnr_at_1k_steps"]["psnr_db_reference_cpu"] = ref["psnr_db"]
                out["psnr_at_1k_steps"]["delta_vs_reference_db"] = out["psnr_at_1k_steps"]["psnr_db"] - ref["psnr_db"]
            if snaps and "psnr_at_1k_steps" in out:
                # The reference run's PSNR at every read step: the ORACLE's weights at that step through the evaluation
                # chain (forward sweep + reconstruction + PSNR, tests/test_gpu_parity.py holds it to the oracle's chain;
                # the read at the last step is ALSO evaluated by the oracle's own chain on the CPU, above: the two agree)
                ev = INRTrainer(dict(cfg), image, coords, shape, dev, seed=0)
                ref_reads = {}
                for k_, sd_ in sorted(snaps.items()):
                    ev.model.load_state_dict({n_: v.to(dev) for n_, v in sd_.items()})
                    ev.engine.pack()
                    ref_reads[k_] = ev.evaluate()
                del ev
                out["psnr_at_1k_steps"]["reference_weights_read_at_last_step_db"] = ref_reads.get(args.psnr_steps)
                out["psnr_at_1k_steps"]["last_epoch"] = psnr_summary(f32_reads, coil_steps, ref_reads)
                out["psnr_at_1k_steps"]["last_epoch_reference"] = psnr_summary(ref_reads, coil_steps)
                out["_ref_reads"] = ref_reads
                out["_coil_steps"] = coil_steps
    if args.full and world == 1 and rank == 0 and args.batch != 65536:  # after the PSNR read-out: these steps keep fitting
        # SURVEY.md 8(d) / north-star point: the same kernel and the same whole step at 65 536 coordinates
        # (2048 wave tiles = two full rounds of the chip's 1024 SIMDs, no tail)
        nsb = 65536
        xs, gs = tr.coords[:nsb], tr.image[:nsb]

        def ns_step():
            eng.train_step(xs, tr.enc_B, gs, tr.loss)
            eng.adam_step(cfg["lr"], 0.9, 0.999, 1e-8, 0.0)

        for _ in range(200):  # (this section follows ~70 s of CPU-only work: let the clocks come back up first)
            ns_step()
        ns_ms = fused_kernel_ms(nsb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(100):
            ns_step()
        torch.cuda.synchronize()
        ns_dt = (time.perf_counter() - t1) / 100
        ns_ach = FLOP_FUSED_F32 * nsb / (ns_ms * 1e-3) / 1e12
        ns_p = gradient_path_ms(nsb)
        ns_pach = FLOP_PER_SAMPLE * nsb / (ns_p * 1e-3) / 1e12
        out["batch_65536"] = {"kernel": fused_kernel_name(nsb), "kernel_ms": ns_ms, "achieved": ns_ach, "frac": ns_ach / F32_MFMA_PEAK_TFLOPS,
                              "unit": "TFLOP/s", "gradient_path_ms": ns_p,
                              "gradient_path_frac": ns_pach / F32_MFMA_PEAK_TFLOPS,
                              "ms_per_step": ns_dt * 1e3, "coord_samples_per_s": nsb / ns_dt}
    # The objects below ride in the same line but are not the graded metric: a failure in one of them is reported in its
    # place ({"error": ...}, also on stderr) instead of taking the line -- and the driver's measurement -- down with it.
    def secondary(name, fn):
        try:
            return fn()
        except Exception as e:  # noqa: BLE001
            import traceback
            traceback.print_exc(file=sys.stderr)
            return {"error": f"{name}: {type(e).__name__}: {e}"}

    if args.full and world == 1 and rank == 0 and not args.no_bf16:
        out["bf16_path"] = secondary("bf16_path", lambda: bf16_path(cfg, image, coords, shape, dev, args, fused_kernel_ms_of, out))
        ref = out.get("cpu_baseline", {}).get("reference_psnr")
        if ref is not None and "psnr_at_1k_steps" in out["bf16_path"]:
            out["bf16_path"]["psnr_at_1k_steps"]["delta_vs_reference_db"] = (
                out["bf16_path"]["psnr_at_1k_steps"]["psnr_db"] - ref["psnr_db"])
    if args.full and world == 1 and rank == 0 and not args.no_config5:
        out["config5_percoil_tv"] = secondary("config5_percoil_tv", lambda: config5_percoil(dev))
    if args.full and not args.no_multiscale:  # every rank takes part (strong scaling over the world)
        ms = secondary("multiscale_config4", lambda: multiscale_config4(dev, rank, world, pg, args.ms_steps, 3, barrier))
        if rank == 0:
            out["multiscale_config4"] = ms
    if rank == 0:
        out.pop("_ref_reads", None)
        out.pop("_coil_steps", None)
        print(json.dumps(out))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
