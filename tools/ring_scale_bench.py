"""Measures ring-normalised fits on one MI355X and writes profiles/ring_norm.json (recorded, not gated).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace), four rings (the k-means partition) and 40 rings:
  * device time of one inr_ring_scale call: --batch calls are enqueued back to back through the C entry itself
    (arguments built beforehand) between ONE pair of device events and the window's time is divided by the batch; median
    of --repeats windows after --warmup.  The buffers rotate over enough copies to exceed the 256 MiB Infinity Cache, so
    every call streams from HBM.  Where the host enqueues more slowly than the device runs it is an upper bound;
  * its 20 bytes per row / time as a fraction of the device-to-device copy rate (read + written bytes / time of a
    1 GiB copy) measured in the same run the same way;
  * beside it, the reference's way in torch on the same resident tensors: K masked index assignments
    (``ind = torch.where((dist >= r0) & (dist < r1)); img[ind] = img[ind] / stat``) -- the baseline, not the code under
    test -- and that both give the same bits.
Fit: BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan with
ring_normalization off, max and min: PSNR / SSIM of validate() and its band report after --epochs epochs in all (the
first one is the warm-up and is left out of the timing), one run each, and seconds per epoch.

Run it under a time limit:  timeout -k 10 900 python tools/ring_scale_bench.py [--epochs 20] [--out FILE]
"""
import argparse
import ctypes
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


def event_times(fn, repeats, warmup):
    """milliseconds of fn(i) per call, by device events"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for i in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def raw_call(dist, vin, out, radii, div):
    from inr_mi355x import _lib as L
    from inr_mi355x.ringnorm import _table
    r32, d32 = _table(radii, div)
    FP = ctypes.POINTER(ctypes.c_float)
    fn, stream = L.load().inr_ring_scale, torch.cuda.current_stream().cuda_stream
    args = (dist.data_ptr(), vin.data_ptr(), out.data_ptr(), dist.numel(), r32.ctypes.data_as(FP), d32.ctypes.data_as(FP),
            int(d32.size), stream)

    def call(keep=(r32, d32)):
        if fn(*args) != 0:
            raise RuntimeError(L.last_error())
    return call


def torch_way(img, dist, radii, stats):
    """scale_space of the reference, in place on ``img``"""
    for i in range(len(radii) - 1):
        ind = torch.where((dist >= radii[i]) & (dist < radii[i + 1]))
        img[ind] = img[ind] / stats[i]
    return img


def kernels(dev, opts):
    from inr_mi355x.ringnorm import RingTable, ring_scale
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    n = C * H * W
    image, coords, _ = make_kspace(C, H, W)
    image, coords = image.to(dev).contiguous(), coords.to(dev)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2).contiguous()
    res = {"shape": list(SHAPE), "rows": n, "bytes_per_row": 20}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    t4 = RingTable.from_rows(image, dist, 40, 4, "max")
    r40 = np.sqrt(2.0) * np.arange(41) / 40.0
    r40[40] = 5.0
    d40 = np.exp(np.random.default_rng(0).uniform(-6, 0, 40)).astype(np.float32)
    res["table4"] = t4.summary()
    copies = max(2, -(-(300 << 20) // (n * 20)))
    sets = [(dist.clone(), image.clone(), torch.empty_like(image)) for _ in range(copies)]
    res["buffer_copies_in_rotation"] = copies
    for name, radii, div in (("rings4", t4.radii, t4.divisors), ("rings40", r40, d40)):
        calls = [raw_call(d, v, o, radii, div) for d, v, o in sets]

        def window(i, calls=calls):
            for k in range(opts.batch):
                calls[(i * opts.batch + k) % copies]()
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(calls_per_window=opts.batch, rings=len(div), bytes=n * 20, bytes_per_s=n * 20 / (t["median_ms"] * 1e-3))
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        stats = torch.from_numpy(np.asarray(div, dtype=np.float32)).to(dev)
        work = image.clone()

        def masked(i):
            work.copy_(image)
            torch_way(work, dist, radii, stats)
        restore = summary(event_times(lambda i: work.copy_(image), opts.torch_repeats, 2))
        tw = summary(event_times(masked, opts.torch_repeats, 2))
        t["torch_masked_assignments"] = dict(tw, median_ms_less_restore=tw["median_ms"] - restore["median_ms"])
        t["torch_over_kernel"] = t["torch_masked_assignments"]["median_ms_less_restore"] / t["median_ms"]
        t["same_bits_as_torch"] = bool(torch.equal(ring_scale(dist, image, radii, div).view(torch.int32),
                                                   work.view(torch.int32)))
        res[name] = t
        print(name, json.dumps(t), flush=True)
    return res


def fit(dev, key, epochs):
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train import INRTrainer, set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(undersampling=None, ring_normalization=key)
    opts = argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE))
    image, coords, shape, cc = cli_fit_data(opts, cfg, "coil")
    tr = INRTrainer(cfg, image, coords, shape, dev, coil_compression=cc)
    tr.enable_band_report(10)
    steps = tr.steps_per_epoch
    tr.fit(steps)  # one epoch of warm-up (allocations, first launches); it counts as a fitted epoch
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps * epochs)
    torch.cuda.synchronize()
    seconds = (time.time() - t0) / (epochs - 1)
    rec = tr.validate(epochs - 1)
    return {"ring_normalization": key, "table": rec.get("ring_normalization"), "steps_per_epoch": steps, "epochs": epochs,
            "seconds_per_epoch": seconds, "psnr": rec["psnr"], "ssim": rec["ssim"], "test_loss": rec["test_loss"],
            "bands_err_db": [b["err_db"] for b in rec["bands"]], "bands_lo": [b["lo"] for b in rec["bands"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=400, help="back-to-back calls per timed window")
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ring_norm.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ring_scale_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernels(dev, opts), "fits": []}
    for key in ("none", "max", "min"):
        try:
            res["fits"].append(fit(dev, key, opts.epochs))
        except ValueError as e:  # a ring whose statistic is zero cannot be divided by: recorded, like any other figure
            res["fits"].append({"ring_normalization": key, "error": str(e)})
        print(json.dumps(res["fits"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
