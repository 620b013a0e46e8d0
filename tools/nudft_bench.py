"""Measures off-grid sampling on one MI355X and writes profiles/nudft.json (recorded, not gated).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace, coil images by evalchain.ifft2c) for spokes-92
(58 880 samples per coil, acceleration 4): HIP events around back-to-back inr_nudft calls after a warm-up, three windows,
the median reported with all three listed; the FLOP of the contraction it performs (8 real FLOP per complex
multiply-add: M W C H for T, M C H for the sum over rows) and the share that gives of the fp32 matrix pipe's peak
(157.3 TFLOP/s, v_mfma_f32_16x16x4_f32).  In the same process, the same contraction as torch complex matmuls on
precomputed complex64 tables ((Ex @ I_c^T) * Ey summed over rows, per coil) -- the baseline, not the code under test.
Accuracy: max |out - ref| / bound of the tests' formula on a 3 x 64 x 48 sub-problem against trajectory.nudft_numpy.
Fit: BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan with
trajectory: spokes-92 + shuffle against undersampling: radial-4 + shuffle, at the same number of optimizer steps (the
learning-rate schedule of each stretched over its own epochs), PSNR / SSIM of validate() on the full grid for both.

Run it under a time limit:  timeout -k 10 900 python tools/nudft_bench.py [--steps 2820] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

SHAPE = (15, 640, 368)
SPOKES = 92
FP32_MATRIX_PEAK = 157.3e12


def windows(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return {"reps_per_window": reps, "seconds_windows": times, "seconds": statistics.median(times)}


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
    scratch = torch.empty(T.scratch_floats(C, H, W, M), device=dev)
    out = torch.empty(C, M, 2, device=dev)
    lib, st = L.load(), torch.cuda.current_stream(dev).cuda_stream
    r = windows(lambda: L.check(lib.inr_nudft(img.data_ptr(), C, H, W, pos.data_ptr(), M, out.data_ptr(),
                                              scratch.data_ptr(), scratch.numel(), st)), reps=5)
    r.update(shape=list(SHAPE), trajectory="spokes-%d" % SPOKES, rows_per_coil=M, acceleration=H * W / M,
             scratch_bytes=scratch.numel() * 4, flop=8 * M * C * H * (W + 1))
    r["tflops"] = r["flop"] / r["seconds"] / 1e12
    r["share_of_fp32_matrix_peak"] = r["flop"] / r["seconds"] / FP32_MATRIX_PEAK
    # the same contraction in torch, on tables made beforehand (complex64)
    ex = torch.from_numpy(T._phasors(pos_np[:, 1], W).astype(np.complex64)).to(dev)
    ey = torch.from_numpy((T._phasors(pos_np[:, 0], H) / math.sqrt(H * W)).astype(np.complex64)).to(dev)
    ic = torch.view_as_complex(img)

    def torch_form():
        return torch.stack([((ex @ ic[c].T) * ey).sum(dim=1) for c in range(C)])

    t = windows(torch_form, reps=3)
    ref = torch_form()
    got = torch.view_as_complex(out)
    t["max_abs_difference_to_kernel"] = float((ref - got).abs().max())
    t["kernel_time_ratio"] = r["seconds"] / t["seconds"]
    return {"inr_nudft": r, "torch_complex_matmul": t}


def accuracy(dev):
    from inr_mi355x import trajectory as T
    C, H, W = 3, 64, 48
    g = np.random.default_rng(0)
    img = (g.standard_normal((C, H, W)) + 1j * g.standard_normal((C, H, W))).astype(np.complex64)
    pos = np.concatenate([T.spokes(H, W, 8), g.uniform(-H, 2 * H, size=(500, 2))])
    pairs = torch.from_numpy(np.stack([img.real, img.imag], -1)).to(dev)
    got = torch.view_as_complex(T.nudft(pairs, pos).cpu()).numpy().astype(np.complex128)
    err = np.abs(got - T.nudft_numpy(img, pos)) / T.error_bound(img, H, W)[:, None]
    return {"shape": [C, H, W], "positions": int(pos.shape[0]), "max_error_over_bound": float(err.max())}


def fit(dev, steps, **switch):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer, set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(dict(undersampling=None, shuffle=True), **switch)
    image, coords, shape = make_kspace(*SHAPE, normalization=cfg["normalization"])
    rows = SHAPE[0] * (SPOKES * max(SHAPE[1:]) if "trajectory" in switch else SHAPE[1] * SHAPE[2])
    cfg["max_epoch"] = math.ceil(steps / math.ceil(rows / cfg["batch_size"]))
    tr = INRTrainer(cfg, image, coords, shape, dev)
    t0 = time.time()
    tr.fit(steps)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rec = tr.validate(cfg["max_epoch"] - 1)
    return dict(switch, steps=tr.global_step, steps_per_epoch=tr.steps_per_epoch, epochs=cfg["max_epoch"],
                training_rows=int(tr.n_train), sampled_rows=int(tr.n_train if tr.mask is None else tr.mask.sum()),
                seconds=seconds, psnr=rec["psnr"], ssim=rec["ssim"], test_loss=rec["test_loss"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2820)  # 20 epochs of the grid fit
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nudft.json"))
    opts = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_flops": FP32_MATRIX_PEAK}
    res["accuracy"] = accuracy(dev)
    print(json.dumps(res["accuracy"]), flush=True)
    res["kernel"] = kernel(dev)
    print(json.dumps(res["kernel"]), flush=True)
    torch.cuda.empty_cache()
    res["fits"] = [fit(dev, opts.steps, trajectory="spokes-%d" % SPOKES), fit(dev, opts.steps, undersampling="radial-4")]
    res["fits"][0]["psnr_minus_radial"] = res["fits"][0]["psnr"] - res["fits"][1]["psnr"]
    for f in res["fits"]:
        print(json.dumps(f), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
