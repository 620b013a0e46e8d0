"""Measures off-grid SENSE fits on calibrated maps on one MI355X and writes profiles/sense_nufft.json (recorded, not gated;
DESIGN.md 4.31).  The timing method is tools/sense_calib_bench.py's: --batch calls enqueued back to back between ONE pair
of device events, the window's time divided by the batch, median of --repeats windows after --warmup; rates as fractions
of the device-to-device copy rate measured in the same run the same way.

Kernels, at the brain shape 15 x 640 x 368 with spokes-92 (M = 58 880 samples per coil), through the C entries on buffer
sets that rotate over more than the 256 MiB Infinity Cache: inr_sense_nufft_prepare (bytes per pixel: 8 img + 8 G maps read,
32 G grid written), inr_sense_nufft_finish (8 G maps + 8 G grid cells read, 8 written: the three quarters of the grid that
are padding are not touched), inr_nufft_interp_plain and inr_nufft_spread_plain (times only: gathers).
Operators, through the Python wrappers a step calls, FFT included, in the same run: sense_nufft against
sense_apply(shift 0) + trajectory.nufft, and sense_nufft_adjoint against trajectory.nufft_adjoint + sense_adjoint(shift 0),
every reusable buffer (scratch, bins, apodisation) handed in on both sides.
Step: one off-grid step with all 15 coils under trajectory_operator gridding and under exact, wall clock with a device
synchronisation, alternating.
Fit, one run: configs/config_siren_sense_radial.yaml (spokes-92, cg-10 from the same samples) for --epochs steps.

Run it under a time limit:  timeout -k 10 900 python tools/sense_nufft_bench.py [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from sense_bench import SCALE, SHAPE, _config, event_times, summary  # noqa: E402
from sense_calib_bench import timed_fit, wall_steps  # noqa: E402

TRAJECTORY = "spokes-92"
# the Cartesian calibrated fit's README line (profiles/sense_calib.json: grid-3*2 plus the 24 x 24 centre, 1000 steps)
CARTESIAN_LINE = {"fit_psnr": 47.14, "fit_ssim": 0.663, "cg10_psnr": 53.19, "cg10_ssim": 0.878, "acceleration": 5.91}


def _timed(window, opts, **extra):
    t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
    t.update(calls_per_window=opts.batch, **extra)
    return t


def kernels(dev, opts, res):
    from inr_mi355x import _lib as L
    from inr_mi355x import trajectory as T
    C, H, W = SHAPE
    n = H * W
    lib, stream, s = L.load(), torch.cuda.current_stream().cuda_stream, ctypes.c_float(SCALE)
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    pos = T.positions(T.parse_trajectory(TRAJECTORY), H, W)
    M = int(pos.shape[0])
    res.update(pixels=n, coils=C, samples_per_coil=M, trajectory=TRAJECTORY)
    d_pos = torch.from_numpy(pos).to(dev)
    ay, ax = T.nufft_device_apodisation(H, W, dev)
    bin_start, order = T.nufft_device_bins(pos, H, W, dev)
    need = T.nufft_scratch_floats(C, H, W, M)
    nbytes = {"prepare": n * (8 + 8 * C + 32 * C), "finish": n * (16 * C + 8)}
    copies = 3  # 3 x 113 MB of grid: more than the Infinity Cache
    sets = []
    for _ in range(copies):
        t = dict(img=torch.empty(n, 2, device=dev).normal_(), maps=torch.empty(C * n, 2, device=dev).normal_(0, 0.3),
                 grid=torch.empty(C, 2 * H, 2 * W, 2, device=dev).normal_(), val=torch.empty(C, M, 2, device=dev).normal_(),
                 out=torch.empty(C, M, 2, device=dev), dimg=torch.empty(n, 2, device=dev),
                 grid_out=torch.empty(C, 2 * H, 2 * W, 2, device=dev), scratch=torch.empty(need, device=dev))
        p = {k: v.data_ptr() for k, v in t.items()}
        calls = {
            "prepare": (lib.inr_sense_nufft_prepare, (p["img"], p["maps"], ay.data_ptr(), ax.data_ptr(), C, H, W, s,
                                                      p["grid_out"], stream)),
            "finish": (lib.inr_sense_nufft_finish, (p["grid"], p["maps"], ay.data_ptr(), ax.data_ptr(), C, H, W, s,
                                                    p["dimg"], 0, stream)),
            "interp_plain": (lib.inr_nufft_interp_plain, (p["grid"], d_pos.data_ptr(), C, H, W, M, p["out"], p["scratch"],
                                                          need, stream)),
            "spread_plain": (lib.inr_nufft_spread_plain, (p["val"], d_pos.data_ptr(), None, bin_start.data_ptr(),
                                                          order.data_ptr(), C, H, W, M, p["grid_out"], p["scratch"], need,
                                                          stream)),
        }
        sets.append((t, calls))
    for name in ("prepare", "finish", "interp_plain", "spread_plain"):
        def window(i, name=name):
            for k in range(opts.batch):
                fn, args = sets[(i * opts.batch + k) % copies][1][name]
                if fn(*args) != 0:
                    raise RuntimeError(L.last_error())
        t = _timed(window, opts, buffer_copies_in_rotation=copies)
        if name in nbytes:
            t.update(bytes=nbytes[name], bytes_per_s=nbytes[name] / (t["median_ms"] * 1e-3))
            t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        res[name] = t
        print(name, json.dumps(t), flush=True)
    del sets


def operators(dev, opts, res):
    """the whole operators as a step calls them, fused against the composition of existing calls, in one run"""
    from inr_mi355x import trajectory as T
    from inr_mi355x.sense import sense_apply
    from inr_mi355x.sense_calib import sense_adjoint
    from inr_mi355x.sense_nufft import SenseNufft
    C, H, W = SHAPE
    n = H * W
    pos = T.positions(T.parse_trajectory(TRAJECTORY), H, W)
    maps = torch.empty(C, n, 2, device=dev).normal_(0, 0.3)
    img = torch.empty(n, 2, device=dev).normal_()
    op = SenseNufft(maps, pos, SHAPE, SCALE, None)
    gk = torch.empty(C, op.M, 2, device=dev).normal_()
    x = torch.empty(C, H, W, 2, device=dev)
    coil = torch.empty(C, H, W, 2, device=dev)
    dimg = torch.empty(n, 2, device=dev)
    out = torch.empty(C, op.M, 2, device=dev)

    def composed_forward():
        sense_apply(img, op.maps, C, H, W, SCALE, 0, out=x)
        return T.nufft(x, op.pos, scratch=op.scratch, apod=op.apod)

    def composed_adjoint():
        T.nufft_adjoint(gk, op.pos, (H, W), None, scratch=op.scratch, out=coil, bins=op.bins, apod=op.apod)
        return sense_adjoint(op.maps, coil, C, H, W, SCALE, 0, dimg=dimg)

    calls = {"fused_forward": lambda: op.forward(img, out=out), "composed_forward": composed_forward,
             "fused_adjoint": lambda: op.adjoint(gk, dimg=dimg), "composed_adjoint": composed_adjoint}
    for name, fn in calls.items():
        def window(i, fn=fn):
            for _ in range(opts.op_batch):
                fn()
        t = summary([ms / opts.op_batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t["calls_per_window"] = opts.op_batch
        res[name] = t
        print(name, json.dumps(t), flush=True)
    res["forward_fused_over_composed"] = res["fused_forward"]["median_ms"] / res["composed_forward"]["median_ms"]
    res["adjoint_fused_over_composed"] = res["fused_adjoint"]["median_ms"] / res["composed_adjoint"]["median_ms"]


def _dump(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=1000, help="epochs (= steps) of the fit")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back kernel calls per timed window")
    ap.add_argument("--op-batch", type=int, default=50, help="back-to-back operator calls per timed window")
    ap.add_argument("--step-repeats", type=int, default=12)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sense_nufft.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sense_nufft_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernel": {}, "operator": {}}
    kernels(dev, opts, res["kernel"])
    _dump(res, opts.out)
    operators(dev, opts, res["operator"])
    _dump(res, opts.out)
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train_sense import SenseFitTrainer
    cfg = _config("config_siren_sense_radial.yaml")
    no_cg = dict(cfg, sense={k: v for k, v in cfg["sense"].items() if k != "baseline"})
    image, coords, shape, _ = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), cfg, "coil")
    new = lambda c: SenseFitTrainer(c, image, coords, shape, dev)
    res["step"] = wall_steps({"gridding": new(no_cg), "exact": new(dict(no_cg, trajectory_operator="exact"))},
                             opts.step_repeats)
    res["step"]["gridding_over_exact"] = res["step"]["gridding"]["median_ms"] / res["step"]["exact"]["median_ms"]
    print("step", json.dumps(res["step"]), flush=True)
    _dump(res, opts.out)
    tr = new(cfg)
    fit = timed_fit(tr, "offgrid_calibrated_" + TRAJECTORY, steps=opts.epochs)
    fit["trajectory"] = tr.trajectory_info
    res["fits"] = [fit, dict(CARTESIAN_LINE, fit="cartesian_calibrated_readme_line")]
    print(json.dumps(fit), flush=True)
    _dump(res, opts.out)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
