"""Measures the continuous ring divisor on one MI355X and writes profiles/ring_profile.json (recorded, not gated).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace), taken the way tools/ring_scale_bench.py takes its
numbers (its event_times / raw_call are imported): --batch calls enqueued back to back through the C entry between one
pair of device events, median of --repeats windows after --warmup, buffers rotating over more than the 256 MiB Infinity
Cache so that every call streams from HBM:
  * one inr_radial_scale call, 1024 knots, dividing and multiplying;
  * inr_ring_scale with the four rings of the same k-means table, in the same run;
  * the device-to-device copy rate (read + written bytes / time of a 1 GiB copy) in the same run, the kernel's 20 bytes
    per row / time as a fraction of it, and the ratio to the step kernel;
  * the same call with the rows in a random order (the gather's worst case) and with 4096 knots.
Fit: BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000; --epochs 20 = 2840 steps) under
ring_normalization max with ring_profile step, linear and geometric: PSNR / SSIM of validate(), normalized_max and the band
report, ONE run each.

Run it under a time limit:  timeout -k 10 600 python tools/ring_profile_bench.py [--epochs 20] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402

from ring_scale_bench import SHAPE, event_times, raw_call, summary  # noqa: E402

KNOTS = 1024


def radial_call(dist, vin, out, prof, r_lo, inv_step, multiply):
    from inr_mi355x import _lib as L
    fn, stream = L.load().inr_radial_scale, torch.cuda.current_stream().cuda_stream
    args = (dist.data_ptr(), vin.data_ptr(), out.data_ptr(), dist.numel(), prof.data_ptr(), prof.numel(), float(r_lo),
            float(inv_step), int(multiply), stream)

    def call():
        if fn(*args) != 0:
            raise RuntimeError(L.last_error())
    return call


def kernels(dev, opts):
    from inr_mi355x.ringnorm import RingTable, ring_profile
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    n = C * H * W
    image, coords, _ = make_kspace(C, H, W)
    image, coords = image.to(dev).contiguous(), coords.to(dev)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2).contiguous()
    res = {"shape": list(SHAPE), "rows": n, "bytes_per_row": 20, "knots": KNOTS}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    t4 = RingTable.from_rows(image, dist, 40, 4, "max")
    res["table4"] = t4.summary()
    copies = max(2, -(-(300 << 20) // (n * 20)))
    sets = [(dist.clone(), image.clone(), torch.empty_like(image)) for _ in range(copies)]
    perm = torch.randperm(n, device=dev, generator=torch.Generator(dev).manual_seed(0))
    shuffled = [(d[perm].contiguous(), v, o) for d, v, o in sets]
    res["buffer_copies_in_rotation"] = copies

    def timed(name, calls, **extra):
        def window(i):
            for k in range(opts.batch):
                calls[(i * opts.batch + k) % copies]()
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(calls_per_window=opts.batch, bytes=n * 20, bytes_per_s=n * 20 / (t["median_ms"] * 1e-3), **extra)
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        res[name] = t
        print(name, json.dumps(t), flush=True)
        return t

    def profile(knots):
        p, r_lo, inv_step = ring_profile(t4.radii, t4.divisors, "geometric", knots)
        return torch.from_numpy(p).to(dev), r_lo, inv_step

    p1k, p4k = profile(KNOTS), profile(4096)
    # alternate the two kernels under comparison: step, radial, step again
    step_a = timed("ring_scale_rings4", [raw_call(d, v, o, t4.radii, t4.divisors) for d, v, o in sets], rings=4)
    rad = timed("radial_scale", [radial_call(d, v, o, *p1k, 0) for d, v, o in sets], knots=KNOTS, multiply=0)
    step_b = timed("ring_scale_rings4_again", [raw_call(d, v, o, t4.radii, t4.divisors) for d, v, o in sets], rings=4)
    timed("radial_scale_multiply", [radial_call(d, v, o, *p1k, 1) for d, v, o in sets], knots=KNOTS, multiply=1)
    timed("radial_scale_random_rows", [radial_call(d, v, o, *p1k, 0) for d, v, o in shuffled], knots=KNOTS, multiply=0)
    timed("radial_scale_4096_knots", [radial_call(d, v, o, *p4k, 0) for d, v, o in sets], knots=4096, multiply=0)
    timed("radial_scale_4096_knots_random_rows", [radial_call(d, v, o, *p4k, 0) for d, v, o in shuffled], knots=4096,
          multiply=0)
    res["radial_over_step"] = rad["median_ms"] / (0.5 * (step_a["median_ms"] + step_b["median_ms"]))
    res["table_path"] = "LDS (the only one built)"
    return res


def fit(dev, mode, epochs):
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train import INRTrainer, set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(undersampling=None, ring_normalization="max", ring_profile=mode, ring_profile_knots=KNOTS)
    opts = argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE))
    image, coords, shape, cc = cli_fit_data(opts, cfg, "coil")
    tr = INRTrainer(cfg, image, coords, shape, dev, coil_compression=cc)
    tr.enable_band_report(10)
    tr.fit(tr.steps_per_epoch * epochs)
    rec = tr.validate(epochs - 1)
    table = rec.get("ring_normalization") or {}
    return {"ring_normalization": "max", "ring_profile": mode, "single_run": True, "steps": tr.global_step, "table": table,
            "normalized_max": table.get("normalized_max"), "psnr": rec["psnr"], "ssim": rec["ssim"],
            "test_loss": rec["test_loss"], "bands_err_db": [b["err_db"] for b in rec["bands"]],
            "bands_lo": [b["lo"] for b in rec["bands"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=400, help="back-to-back calls per timed window")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ring_profile.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ring_profile_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernels(dev, opts), "fits": []}
    for mode in ("step", "linear", "geometric"):
        try:
            res["fits"].append(fit(dev, mode, opts.epochs))
        except ValueError as e:  # a ring whose statistic is zero cannot be divided by: recorded, like any other figure
            res["fits"].append({"ring_normalization": "max", "ring_profile": mode, "error": str(e)})
        print(json.dumps(res["fits"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
