"""Measures SENSE fits on calibrated coil maps on one MI355X and writes profiles/sense_calib.json (recorded, not gated;
DESIGN.md 4.29).  The timing method is tools/sense_bench.py's: --batch calls enqueued back to back through the C entry
between ONE pair of device events, the window's time divided by the batch, median of --repeats windows after --warmup, on
buffers that rotate over more than the 256 MiB Infinity Cache; rates as fractions of the device-to-device copy rate
measured in the same run the same way.

Kernels, at the brain shape 15 x 640 x 368 with a 24 x 24 block: inr_sense_lowres (bytes: the output, 8 per pixel and
coil -- the block and the tables stay in cache), inr_sense_maps (both launches: 8 C read twice + 8 C + 4 written + 4 read
per pixel), inr_sense_adjoint (16 G + 8 per pixel) and, on the same inputs, inr_sense_grad (16 + 24 G).
Step: one calibrated step with all 15 coils against one learned-maps step with 5 (configs/config_siren_sense.yaml; the
learned path is the parent's code, untouched), wall clock with a device synchronisation, alternating, per step and per
epoch (1 against 3 steps).
Fits, one run each, same mask rule (grid-3*2; the calibrated fit adds the 24 x 24 centre): the calibrated fit for
--epochs epochs with its cg-10 baseline, the learned-maps fit for the same wall-clock time, the plain fit for
--plain-epochs epochs, the zero-filled RSS of the calibrated fit's mask.

Run it under a time limit:  timeout -k 10 900 python tools/sense_calib_bench.py [--out FILE]
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
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from sense_bench import SCALE, SHAPE, _config, event_times, summary, zero_filled  # noqa: E402

BLOCK = (24, 24)


def kernels(dev, opts):
    from inr_mi355x import _lib as L
    from inr_mi355x import sense_calib as K
    C, H, W = SHAPE
    n, (a, b) = H * W, BLOCK
    lib, stream, s = L.load(), torch.cuda.current_stream().cuda_stream, ctypes.c_float(SCALE)
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res = {"pixels": n, "coils": C, "block": list(BLOCK), "copy": dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)}
    del src, dst
    ey, ex = (torch.from_numpy(t).to(dev) for t in K.grid_tables(H, W, a, b))
    nbytes = {"lowres": n * C * 8, "maps": n * (24 * C + 8), "adjoint": n * (16 * C + 8), "grad": n * (16 + 24 * C)}
    copies = max(2, -(-(300 << 20) // nbytes["lowres"]))
    sets = []
    for _ in range(copies):
        t = dict(block=torch.empty(C, a, b, 2, device=dev).normal_(0, 0.3), low=torch.empty(C, n, 2, device=dev).normal_(),
                 maps=torch.empty(C, n, 2, device=dev), rss=torch.empty(n, device=dev),
                 gx=torch.empty(C, H, W, 2, device=dev).normal_(0, 0.3), img=torch.empty(n, 2, device=dev).normal_(),
                 dimg=torch.empty(n, 2, device=dev), dsens=torch.empty(C * n, 2, device=dev))
        p = {k: v.data_ptr() for k, v in t.items()}
        calls = {
            "lowres": (lib.inr_sense_lowres, (p["block"], ey.data_ptr(), ex.data_ptr(), C, a, b, H, W, p["maps"], stream)),
            "maps": (lib.inr_sense_maps, (p["low"], C, n, ctypes.c_float(0.0), p["maps"], p["rss"], stream)),
            "adjoint": (lib.inr_sense_adjoint, (p["low"], p["gx"], C, H, W, s, 1, p["dimg"], stream)),
            "grad": (lib.inr_sense_grad, (p["img"], p["low"], p["gx"], C, H, W, s, 1, p["dimg"], p["dsens"], stream)),
        }
        sets.append((t, calls))
    for name in ("lowres", "maps", "adjoint", "grad"):
        def window(i, name=name):
            for k in range(opts.batch):
                fn, args = sets[(i * opts.batch + k) % copies][1][name]
                if fn(*args) != 0:
                    raise RuntimeError(L.last_error())
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(bytes=nbytes[name], bytes_per_s=nbytes[name] / (t["median_ms"] * 1e-3), calls_per_window=opts.batch,
                 buffer_copies_in_rotation=copies)
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        res[name] = t
        print(name, json.dumps(t), flush=True)
    res["adjoint_over_grad"] = res["adjoint"]["median_ms"] / res["grad"]["median_ms"]
    return res


def wall_steps(trainers, repeats):
    """wall-clock milliseconds per step of each trainer, alternating between them, synchronised around every step"""
    out = {name: [] for name in trainers}
    for name, tr in trainers.items():  # warm-up: one epoch each
        for it in range(tr.steps_per_epoch):
            tr.step(0, it)
    for r in range(repeats):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(0, r % tr.steps_per_epoch)
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for name, tr in trainers.items():
        res[name] = dict(summary(out[name]), coils_per_step=tr.coils_per_step, steps_per_epoch=tr.steps_per_epoch)
        res[name]["epoch_ms"] = res[name]["median_ms"] * tr.steps_per_epoch
    return res


def timed_fit(tr, name, steps=None, seconds=None):
    """fit for ``steps`` steps, or until ``seconds`` of wall clock have passed (checked every epoch)"""
    torch.cuda.synchronize()
    t0 = time.time()
    if steps is not None:
        tr.fit(steps)
    else:
        epoch = 0
        while time.time() - t0 < seconds and epoch < tr.config["max_epoch"]:
            for it in range(tr.steps_per_epoch):
                tr.step(epoch, it)
            torch.cuda.synchronize()
            epoch += 1
    torch.cuda.synchronize()
    spent = time.time() - t0
    rec = tr.metrics()
    return {"fit": name, "steps": tr.global_step, "seconds": spent, "psnr": rec["psnr"], "ssim": rec["ssim"],
            "sense": rec.get("sense"), "cg_sense": rec.get("cg_sense")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=1000, help="epochs (= steps) of the calibrated fit")
    ap.add_argument("--plain-epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--step-repeats", type=int, default=12)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sense_calib.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sense_calib_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernel": kernels(dev, opts)}
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_sense import SenseFitTrainer
    learned_cfg, calib_cfg = _config("config_siren_sense.yaml"), _config("config_siren_sense_calibrated.yaml")
    image, coords, shape, _ = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), calib_cfg, "coil")
    new = lambda cfg: SenseFitTrainer(cfg, image, coords, shape, dev)
    res["step"] = wall_steps({"calibrated": new(calib_cfg), "learned": new(learned_cfg)}, opts.step_repeats)
    print("step", json.dumps(res["step"]), flush=True)
    res["fits"] = []
    tr = new(calib_cfg)
    res["fits"].append(timed_fit(tr, "calibrated", steps=opts.epochs * tr.steps_per_epoch))
    res["fits"].append(dict(zero_filled(tr), mask="grid-3*2 + 24 x 24 centre", acceleration=tr.acceleration))
    seconds = res["fits"][0]["seconds"]
    del tr
    res["fits"].append(timed_fit(new(learned_cfg), "learned_same_wall_clock", seconds=seconds))
    plain = {k: v for k, v in learned_cfg.items() if k != "sense"}
    tr = INRTrainer(plain, image, coords, shape, dev)
    res["fits"].append(timed_fit(tr, "plain", steps=opts.plain_epochs * tr.steps_per_epoch))
    for f in res["fits"]:
        print(json.dumps(f), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
