"""Measures coil compression on one MI355X and writes profiles/coil_compress.json (recorded, not gated).

Kernels, at the brain shape 15 x 640 x 368 (synthetic.make_kspace, before normalisation), timed as
tools/reconstruct_bench.py times inr_grid_rows -- HIP events around back-to-back launches after a warm-up, three windows,
the median window reported with all three listed:
  * inr_coil_gram (15 coils) and inr_coil_apply (15 -> 8), with the bytes each must move and the rate that gives;
  * in the same run, a device-to-device copy of the scan (the HBM rate the two are stated against) and the plain torch
    expressions on the same resident tensors, complex matmul x x^H and A x -- the baseline, not the code under test.
Fit: BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan with
virtual_coils off, 12 and 8: seconds per epoch (host clock around whole epochs that end in a synchronise), PSNR / SSIM of
validate() after the same number of epochs -- each scored against its own (virtual-coil) targets -- and rss_psnr.

Run it under a time limit:  timeout -k 10 900 python tools/coil_compress_bench.py [--epochs 20] [--out FILE]
"""
import argparse
import json
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


def windows(fn, target_s=0.3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    reps = max(10, min(2000, int(target_s / max(time.time() - t0, 1e-6))))
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


def kernels(dev):
    import ctypes
    from inr_mi355x import _lib as L
    from inr_mi355x import coils as CC
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    N = H * W
    x = make_kspace(C, H, W, normalization=None)[0].reshape(C, N, 2).to(dev).contiguous()
    G = CC.coil_gram(x, (C,))
    A = CC.compression_matrix(G, 8)[0]
    lib, st = L.load(), torch.cuda.current_stream(dev).cuda_stream
    gram = torch.empty(C, C, 2, device=dev, dtype=torch.float64)
    scratch = torch.empty(CC.scratch_doubles(C, N), device=dev, dtype=torch.float64)
    a_dev = torch.from_numpy(CC._pairs(A, np.float32)).to(dev)
    y = torch.empty(8, N, 2, device=dev)
    xc, ac = torch.view_as_complex(x), torch.view_as_complex(a_dev)
    copy_dst = torch.empty_like(x)
    out = {"shape": list(SHAPE)}
    r = windows(lambda: L.check(lib.inr_coil_gram(x.data_ptr(), C, N, gram.data_ptr(), scratch.data_ptr(),
                                                  scratch.numel(), st)))
    r["bytes"] = x.numel() * 4 + 2 * scratch.numel() * 8
    out["inr_coil_gram"] = r
    r = windows(lambda: L.check(lib.inr_coil_apply(x.data_ptr(), a_dev.data_ptr(), 8, C, N, y.data_ptr(), st)))
    r["bytes"] = (x.numel() + y.numel()) * 4
    out["inr_coil_apply_15_to_8"] = r
    r = windows(lambda: copy_dst.copy_(x))
    r["bytes"] = 2 * x.numel() * 4
    out["hbm_copy"] = r
    out["torch_gram_complex_matmul"] = windows(lambda: xc @ xc.conj().T)
    out["torch_apply_complex_matmul"] = windows(lambda: ac @ xc)
    for k in ("inr_coil_gram", "inr_coil_apply_15_to_8", "hbm_copy"):
        out[k]["GB_per_s"] = out[k]["bytes"] / out[k]["seconds"] / 1e9
    for k in ("inr_coil_gram", "inr_coil_apply_15_to_8"):
        out[k]["share_of_copy_rate"] = out[k]["GB_per_s"] / out["hbm_copy"]["GB_per_s"]
    out["inr_coil_gram"]["fp64_fma"] = 4 * N * (C * (C + 1) // 2)
    return out


def fit(dev, K, epochs):
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train import INRTrainer, set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(undersampling=None, virtual_coils=K)
    opts = argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE))
    image, coords, shape, cc = cli_fit_data(opts, cfg, "coil")
    tr = INRTrainer(cfg, image, coords, shape, dev, coil_compression=cc)
    steps = tr.steps_per_epoch
    tr.fit(steps)  # one epoch of warm-up (allocations, first launches); it counts as a fitted epoch
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps * epochs)
    torch.cuda.synchronize()
    seconds = (time.time() - t0) / (epochs - 1)
    rec = tr.validate(epochs - 1)
    return {"virtual_coils": K, "coils": int(shape[0]), "rows": int(tr.n), "steps_per_epoch": steps, "epochs": epochs,
            "seconds_per_epoch": seconds, "psnr": rec["psnr"], "ssim": rec["ssim"],
            "rss_psnr": None if cc is None else cc.rss_psnr, "energy_kept": None if cc is None else cc.energy_kept}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "coil_compress.json"))
    opts = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels(dev), "fits": []}
    for K in (0, 12, 8):
        res["fits"].append(fit(dev, K, opts.epochs))
        print(json.dumps(res["fits"][-1]), flush=True)
    base = res["fits"][0]
    for f in res["fits"][1:]:
        f["epoch_time_ratio"] = f["seconds_per_epoch"] / base["seconds_per_epoch"]
        f["psnr_minus_off"] = f["psnr"] - base["psnr"]
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["kernels"]))


if __name__ == "__main__":
    main()
