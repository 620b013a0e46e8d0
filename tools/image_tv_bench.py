"""Measures the total-variation prior on the image of a SENSE fit on one MI355X and writes profiles/image_tv.json
(recorded, not gated).  The timing method is tools/sense_calib_bench.py's: --batch calls enqueued back to
back through the C entry between ONE pair of device events, the window's time divided by the batch, median of --repeats
windows after --warmup; the device-to-device copy rate is measured in the same run the same way.

Kernel, at the brain shape 640 x 368: inr_image_tv_grad in its three modes -- write, accumulate, value only.  Bytes the
algorithm needs per pixel: 8 read (+ 8 written; + 8 read when accumulating); the neighbours' re-reads hit in cache.  Each
call is TWO launches (the gather and the one-thread fold); at 1.9 MB the image stays in L2, so the figure is
launch-bound and the fraction of the copy rate is recorded for what it is.  Beside it, timed the same way on the same
image: the same value and gradient from torch ops and autograd (sense_prior_cases-style slicing and torch.sqrt, forward
and backward), and the value alone under no_grad.
Step: one calibrated step (configs/config_siren_sense_calibrated.yaml) without and with the prior, wall clock with a
device synchronisation, alternating.
Fits, one run each, on the synthetic scan under grid-3*2 plus the 24 x 24 centre, --epochs steps: the calibrated fit
without the prior (with its cg-10 baseline) and with it at the --weights; before them, the norms of the data term's and
the prior's gradient to the image at the initial parameters, which say what a weight means.

Run it under a time limit:  timeout -k 10 600 python tools/image_tv_bench.py [--out FILE]
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

from sense_bench import SHAPE, _config, event_times, summary  # noqa: E402
from sense_calib_bench import timed_fit, wall_steps  # noqa: E402

WEIGHT, EPS = 1e-3, 1e-3


def tv_torch(img, H, W, weight, eps):
    """weight * TV of img [H*W,2] with torch ops: what autograd differentiates"""
    I = img.view(H, W, 2)
    dx = torch.nn.functional.pad(((I[:, 1:] - I[:, :-1]) ** 2).sum(-1), (0, 1))
    dy = torch.nn.functional.pad(((I[1:, :] - I[:-1, :]) ** 2).sum(-1), (0, 0, 0, 1))
    return weight * (torch.sqrt(dx + dy + eps * eps) - eps).sum() / (H * W)


def kernels(dev, opts):
    from inr_mi355x import _lib as L
    _, H, W = SHAPE
    n = H * W
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res = {"pixels": n, "shape": [H, W], "weight": WEIGHT, "eps": EPS, "launches_per_call": 2,
           "copy": dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)}
    del src, dst
    img = torch.empty(n, 2, device=dev).uniform_(-0.3, 0.3)
    dimg, out = torch.zeros(n, 2, device=dev), torch.zeros(L.LOSS_WORDS, device=dev)
    w, e = ctypes.c_float(WEIGHT), ctypes.c_float(EPS)
    modes = {"write": ((img.data_ptr(), H, W, w, e, 0, out.data_ptr(), dimg.data_ptr(), stream), 16 * n),
             "accumulate": ((img.data_ptr(), H, W, w, e, 1, out.data_ptr(), dimg.data_ptr(), stream), 24 * n),
             "value_only": ((img.data_ptr(), H, W, w, e, 0, out.data_ptr(), None, stream), 8 * n)}
    for name, (args, nbytes) in modes.items():
        def window(i, args=args):
            for _ in range(opts.batch):
                if lib.inr_image_tv_grad(*args) != 0:
                    raise RuntimeError(L.last_error())
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(bytes=nbytes, bytes_per_s=nbytes / (t["median_ms"] * 1e-3), calls_per_window=opts.batch)
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        t["time_of_the_bytes_at_copy_rate_ms"] = nbytes / copy_rate * 1e3
        res[name] = t
        print(name, json.dumps(t), flush=True)
    # the same value and gradient from torch ops and autograd, and the value alone
    leaf = img.clone().requires_grad_(True)

    def autograd_window(i):
        for _ in range(opts.batch):
            leaf.grad = None
            tv_torch(leaf, H, W, WEIGHT, EPS).backward()

    def value_window(i):
        with torch.no_grad():
            for _ in range(opts.batch):
                tv_torch(img, H, W, WEIGHT, EPS)

    for name, fn in (("torch_autograd", autograd_window), ("torch_value_only", value_window)):
        t = summary([ms / opts.batch for ms in event_times(fn, opts.repeats, opts.warmup)])
        t["calls_per_window"] = opts.batch
        res[name] = t
        print(name, json.dumps(t), flush=True)
    # both compute the same thing: the kernel's value and gradient against autograd's, fp32 against fp32
    lib.inr_image_tv_grad(*modes["write"][0])
    leaf.grad = None
    v = tv_torch(leaf, H, W, WEIGHT, EPS)
    v.backward()
    res["kernel_vs_torch_fp32"] = {
        "value_rel": abs(float(out[0]) - float(v.detach())) / abs(float(v.detach())),
        "gradient_rel_l2": float((dimg.double() - leaf.grad.double()).norm() / leaf.grad.double().norm())}
    res["write_over_torch_autograd"] = res["write"]["median_ms"] / res["torch_autograd"]["median_ms"]
    res["value_only_over_torch_value_only"] = res["value_only"]["median_ms"] / res["torch_value_only"]["median_ms"]
    return res


def step0_norms(tr):
    """|d data loss / dI| and |d TV / dI| (weight 1) at the initial parameters: the scale the weights are read against"""
    from inr_mi355x.sense_prior import image_tv
    _, H, W = SHAPE
    ib = tr.engine.forward(tr._img_in, tr.enc_B, save=False).clone()
    g = torch.zeros_like(ib)
    tv = float(image_tv(ib, H, W, 1.0, EPS, dimg=g))
    data_loss = float(tr.step(0, 0))  # a calibrated step leaves the data term's dimg in tr._dimg
    data, prior = float(tr._dimg.double().norm()), float(g.double().norm())
    return {"data_loss": data_loss, "tv": tv, "data": data, "tv_weight_1": prior, "balanced_weight": data / prior}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=1000, help="epochs (= steps) of every fit")
    ap.add_argument("--weights", type=str, default="1e-5,1e-4,1e-3,1e-2", help="prior weights of the fits, a decade apart")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--step-repeats", type=int, default=24)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "image_tv.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_tv_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernel": kernels(dev, opts)}
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train_sense import SenseFitTrainer
    base = _config("config_siren_sense_calibrated.yaml")

    def cfg(weight=None):
        c = dict(base)
        c["sense"] = dict(base["sense"]) if weight is None else dict(base["sense"], prior={"kind": "tv", "weight": weight,
                                                                                           "eps": EPS})
        return c

    image, coords, shape, _ = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), base, "coil")
    new = lambda c: SenseFitTrainer(c, image, coords, shape, dev)
    res["step"] = wall_steps({"calibrated": new(cfg()), "calibrated_tv": new(cfg(WEIGHT))}, opts.step_repeats)
    res["step"]["tv_minus_plain_ms"] = res["step"]["calibrated_tv"]["median_ms"] - res["step"]["calibrated"]["median_ms"]
    print("step", json.dumps(res["step"]), flush=True)
    res["step0_image_gradient_norms"] = step0_norms(new(cfg()))
    print("step 0", json.dumps(res["step0_image_gradient_norms"]), flush=True)
    res["fits"] = []
    tr = new(cfg())
    res["fits"].append(timed_fit(tr, "calibrated", steps=opts.epochs * tr.steps_per_epoch))
    del tr
    for weight in (float(v) for v in opts.weights.split(",")):
        tr = new(cfg(weight))
        rec = timed_fit(tr, f"calibrated_tv_{weight:g}", steps=opts.epochs * tr.steps_per_epoch)
        rec["prior"] = tr.metrics()["prior"]
        res["fits"].append(rec)
        del tr
    for f in res["fits"]:
        print(json.dumps(f), flush=True)
    res["note"] = "one run each; synthetic 15 x 640 x 368 scan, grid-3*2 plus the 24 x 24 centre"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
