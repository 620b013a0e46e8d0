"""Measures the adjoint of the off-grid sampling and the conventional baseline on one MI355X and writes
profiles/nudft_adjoint.json (recorded, not gated).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace) for spokes-92 (58 880 samples per coil): HIP events
around back-to-back inr_adjoint_nudft calls (ramp weights) after a warm-up, three windows, the median reported with all
three listed; the FLOP of its contraction (8 real FLOP per complex multiply-add: C H W M, plus C H M for the A operand) and
the share that gives of the fp32 matrix pipe's peak (157.3 TFLOP/s, v_mfma_f32_16x16x4_f32).  In the same process: the
same contraction as torch complex matmuls on precomputed complex64 tables ((conj(Ey) * w v_c)^T @ conj(Ex), per coil) --
the baseline, not the code under test; inr_nudft on the same positions; and trajectory.cg_baseline with 10 iterations
(wall clock around a synchronised call: it reads two scalars back per iteration).
Accuracy: max |out - ref| / bound of the tests' formula on a 3 x 70 x 66 sub-problem against nudft_adjoint_numpy.
Fit: BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) with trajectory: spokes-92 +
shuffle as tools/nudft_bench.py runs it, its PSNR / SSIM of validate() on the full grid beside the 'gridding' records of
trajectory_baseline: adjoint and cg-10 made from the same samples.  One run on a synthetic scan.

Run it under a time limit:  timeout -k 10 600 python tools/nudft_adjoint_bench.py [--steps 2820] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from nudft_bench import FP32_MATRIX_PEAK, SHAPE, SPOKES, windows  # noqa: E402


def kernel(dev):
    from inr_mi355x import _lib as L
    from inr_mi355x import trajectory as T
    from inr_mi355x.evalchain import ifft2c
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    k = make_kspace(C, H, W)[0].reshape(C, H, W, 2).to(dev)
    img = ifft2c(k).contiguous()
    pos_np = T.spokes(H, W, SPOKES)
    M = pos_np.shape[0]
    pos = torch.from_numpy(pos_np).to(dev)
    w_np = T.density_ramp(SPOKES, M // SPOKES, H, W)
    w = torch.from_numpy(w_np).float().to(dev)
    fwd_scratch = torch.empty(T.scratch_floats(C, H, W, M), device=dev)
    adj_scratch = torch.empty(T.adjoint_scratch_floats(C, H, W, M), device=dev)
    val = torch.empty(C, M, 2, device=dev)
    out = torch.empty(C, H, W, 2, device=dev)
    lib, st = L.load(), torch.cuda.current_stream(dev).cuda_stream
    f = windows(lambda: L.check(lib.inr_nudft(img.data_ptr(), C, H, W, pos.data_ptr(), M, val.data_ptr(),
                                              fwd_scratch.data_ptr(), fwd_scratch.numel(), st)), reps=5)
    f.update(flop=8 * M * C * H * (W + 1))
    f["tflops"] = f["flop"] / f["seconds"] / 1e12
    r = windows(lambda: L.check(lib.inr_adjoint_nudft(val.data_ptr(), pos.data_ptr(), w.data_ptr(), C, H, W, M,
                                                      out.data_ptr(), adj_scratch.data_ptr(), adj_scratch.numel(), st)),
                reps=5)
    r.update(shape=list(SHAPE), trajectory="spokes-%d" % SPOKES, rows_per_coil=M, weights="ramp",
             scratch_bytes=adj_scratch.numel() * 4, flop=8 * M * C * H * (W + 1),
             workgroups=C * math.ceil(H / 64) * math.ceil(W / 64))
    r["tflops"] = r["flop"] / r["seconds"] / 1e12
    r["share_of_fp32_matrix_peak"] = r["flop"] / r["seconds"] / FP32_MATRIX_PEAK
    r["time_over_inr_nudft"] = r["seconds"] / f["seconds"]
    # the same contraction in torch, on tables made beforehand (complex64)
    exc = torch.from_numpy(np.conj(T._phasors(pos_np[:, 1], W)).astype(np.complex64)).to(dev)
    eyc = torch.from_numpy((np.conj(T._phasors(pos_np[:, 0], H)) / math.sqrt(H * W)).astype(np.complex64)).to(dev)
    wv = torch.view_as_complex(val) * w[None, :]

    def torch_form():
        return torch.stack([(eyc * wv[c][:, None]).T @ exc for c in range(C)])

    t = windows(torch_form, reps=3)
    t["max_abs_difference_to_kernel"] = float((torch_form() - torch.view_as_complex(out)).abs().max())
    t["kernel_time_ratio"] = r["seconds"] / t["seconds"]
    del exc, eyc, wv
    torch.cuda.empty_cache()

    def cg():
        torch.cuda.synchronize()
        t0 = time.time()
        _, objective = T.cg_baseline(val, pos, SHAPE, w_np, 10)
        torch.cuda.synchronize()
        return time.time() - t0, objective

    cg()
    runs = [cg() for _ in range(3)]
    secs = sorted(s for s, _ in runs)
    c = {"iters": 10, "seconds_runs": [s for s, _ in runs], "seconds": secs[1], "objective": runs[0][1],
         "operator_seconds_expected": 11 * r["seconds"] + 10 * f["seconds"]}
    return {"inr_adjoint_nudft": r, "torch_complex_matmul": t, "inr_nudft": f, "cg_10": c}


def accuracy(dev):
    from inr_mi355x import trajectory as T
    C, H, W = 3, 70, 66
    g = np.random.default_rng(0)
    pos = np.concatenate([T.spokes(H, W, 8), g.uniform(-H, 2 * H, size=(500, 2))])
    M = pos.shape[0]
    val = (g.standard_normal((C, M)) + 1j * g.standard_normal((C, M))).astype(np.complex64)
    w = g.uniform(0.25, 4.0, M).astype(np.float32)
    pairs = torch.from_numpy(np.stack([val.real, val.imag], -1)).to(dev)
    got = torch.view_as_complex(T.nudft_adjoint(pairs, pos, (H, W), w).cpu()).numpy().astype(np.complex128)
    err = np.abs(got - T.nudft_adjoint_numpy(val, pos, H, W, w)) / T.adjoint_error_bound(val, w, H, W)[:, None, None]
    return {"shape": [C, H, W], "positions": int(M), "max_error_over_bound": float(err.max())}


def fit(dev, steps):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer, set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(dict(undersampling=None, shuffle=True, trajectory="spokes-%d" % SPOKES, trajectory_baseline="cg-10"))
    image, coords, shape = make_kspace(*SHAPE, normalization=cfg["normalization"])
    rows = SHAPE[0] * SPOKES * max(SHAPE[1:])
    cfg["max_epoch"] = math.ceil(steps / math.ceil(rows / cfg["batch_size"]))
    tr = INRTrainer(cfg, image, coords, shape, dev)
    cg10 = tr.gridding
    t0 = time.time()
    tr.fit(steps)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rec = tr.validate(cfg["max_epoch"] - 1)
    # the plain adjoint of the same samples, scored the same way
    tr.trajectory_baseline = ("adjoint", 0)
    tr._gridding_baseline()
    return {"trajectory": cfg["trajectory"], "shuffle": True,
            "fit": dict(steps=tr.global_step, epochs=cfg["max_epoch"], training_rows=int(tr.n_train), seconds=seconds,
                        psnr=rec["psnr"], ssim=rec["ssim"]),
            "adjoint": tr.gridding, "cg-10": cg10}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2820)  # as tools/nudft_bench.py
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nudft_adjoint.json"))
    opts = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_flops": FP32_MATRIX_PEAK}
    res["accuracy"] = accuracy(dev)
    print(json.dumps(res["accuracy"]), flush=True)
    res["kernel"] = kernel(dev)
    print(json.dumps(res["kernel"]), flush=True)
    torch.cuda.empty_cache()
    res["fit_and_baselines"] = fit(dev, opts.steps)
    print(json.dumps(res["fit_and_baselines"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
