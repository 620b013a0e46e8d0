"""Measures learned-gain fits on one MI355X and writes profiles/gain.json (recorded, not gated).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace) and at 25 000 rows, L2 loss, with res:
  * device time of one inr_gain_loss_grad call, the method of tools/ring_scale_bench.py: --batch calls are enqueued back
    to back through the C entry itself (arguments built beforehand) between ONE pair of device events and the window's
    time is divided by the batch; median of --repeats windows after --warmup.  The buffers rotate over enough copies to
    exceed the 256 MiB Infinity Cache, so every call streams from HBM.  Where the host enqueues more slowly than the
    device runs (the 25 000-row case) it is an upper bound;
  * its 41 bytes per row / time as a fraction of the device-to-device copy rate (read + written bytes / time of a 1 GiB
    copy) measured in the same run the same way;
  * beside it the torch-op restatement on the same resident tensors (exp, mul, 0.5 MSE, autograd to y and s) -- the
    baseline, not the code under test.
Step, BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan: wall time per
step of ScaledFitTrainer with the default 512 x 8 gain network against the same backbone's INRTrainer as tier-1 calls
(INR_ONE_CALL_STEPS=0) and as its fused one-call step: what the second network costs.
Fit: the same config scaled against plain, same steps and seed: PSNR / SSIM of validate() and its 10-ring band report
after --epochs epochs, one run each.

Run it under a time limit:  timeout -k 10 900 python tools/gain_bench.py [--epochs 20] [--out FILE]
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

import torch  # noqa: E402
import yaml  # noqa: E402

SHAPE = (15, 640, 368)
BYTES_PER_ROW = 41  # y 8, s 4, gt 8 read; res 8, dy 8, ds 4 written; no mask (+1)


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


def raw_call(ld, y, s, gt, res, loss, dy, ds):
    from inr_mi355x import _lib as L
    fn, stream = L.load().inr_gain_loss_grad, torch.cuda.current_stream().cuda_stream
    args = (ctypes.byref(ld), y.data_ptr(), s.data_ptr(), gt.data_ptr(), None, y.shape[0], res.data_ptr(), loss.data_ptr(),
            dy.data_ptr(), ds.data_ptr(), stream)

    def call(keep=ld):
        if fn(*args) != 0:
            raise RuntimeError(L.last_error())
    return call


def torch_way(y, s, gt):
    y, s = y.detach().requires_grad_(True), s.detach().requires_grad_(True)
    res = y * torch.exp(-s)[:, None]
    loss = 0.5 * torch.nn.functional.mse_loss(res, gt)
    return (loss, res) + torch.autograd.grad(loss, (y, s))


def kernels(dev, opts):
    from inr_mi355x import _lib as L
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    image = make_kspace(C, H, W)[0].to(dev).contiguous()
    res = {"bytes_per_row": BYTES_PER_ROW, "loss": "L2", "blocks": 256}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    for name, n in (("brain", C * H * W), ("rows25000", 25000)):
        gt = image[:n].contiguous()
        copies = max(2, -(-(300 << 20) // (n * BYTES_PER_ROW)))
        ld = L.LossDesc(kind=L.LOSS_L2_HALF, eps=1e-3, sigma=2.0, factor=0.5, inv_count=1.0 / n, hdr_A=0.0)
        sets = []
        for _ in range(copies):
            y, s = torch.empty(n, 2, device=dev).normal_(0, 0.3), torch.empty(n, device=dev).uniform_(0, 1)
            sets.append((y, s, gt.clone(), torch.empty_like(y), torch.zeros(L.LOSS_WORDS, device=dev), torch.empty_like(y),
                         torch.empty_like(s)))
        calls = [raw_call(ld, *st) for st in sets]

        def window(i, calls=calls, copies=copies):
            for k in range(opts.batch):
                calls[(i * opts.batch + k) % copies]()
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(rows=n, calls_per_window=opts.batch, buffer_copies_in_rotation=copies, bytes=n * BYTES_PER_ROW,
                 bytes_per_s=n * BYTES_PER_ROW / (t["median_ms"] * 1e-3))
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        y, s, g = sets[0][0], sets[0][1], sets[0][2]
        tw = summary(event_times(lambda i: torch_way(y, s, g), opts.torch_repeats, 2))
        t["torch_ops"] = tw
        t["torch_over_kernel"] = tw["median_ms"] / t["median_ms"]
        res[name] = t
        print(name, json.dumps(t), flush=True)
        del sets, calls
    return res


def _config():
    from inr_mi355x.trainer_base import set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(undersampling=None)
    return cfg


def _trainer(dev, scaled, data, one_call=True):
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_scaling import ScaledFitTrainer
    image, coords, shape, cc = data
    if scaled:
        return ScaledFitTrainer(_config(), image, coords, shape, dev, coil_compression=cc)
    old = os.environ.get("INR_ONE_CALL_STEPS")
    os.environ["INR_ONE_CALL_STEPS"] = "1" if one_call else "0"  # read by the constructor
    try:
        return INRTrainer(_config(), image, coords, shape, dev, coil_compression=cc)
    finally:
        if old is None:
            del os.environ["INR_ONE_CALL_STEPS"]
        else:
            os.environ["INR_ONE_CALL_STEPS"] = old


def step_times(dev, data, opts):
    """wall milliseconds per step over windows of --step-window steps of epoch 0 (full batches of 25 000 rows)"""
    out = {}
    for name, scaled, one_call in (("scaled_512x8", True, True), ("plain_tier1_two_calls", False, False),
                                   ("plain_fused_one_call", False, True)):
        tr = _trainer(dev, scaled, data, one_call)
        n = min(opts.step_window, tr.steps_per_epoch - 1)
        for it in range(n):  # warm-up: allocations, first launches
            tr.step(0, it)
        ms = []
        for _ in range(opts.step_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(n):
                tr.step(0, it)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / n)
        out[name] = dict(summary(ms), steps_per_window=n, batch=tr.bs)
        print(name, json.dumps(out[name]), flush=True)
        del tr
    out["scaled_over_tier1"] = out["scaled_512x8"]["median_ms"] / out["plain_tier1_two_calls"]["median_ms"]
    out["scaled_over_fused"] = out["scaled_512x8"]["median_ms"] / out["plain_fused_one_call"]["median_ms"]
    return out


def fit(dev, scaled, data, epochs):
    tr = _trainer(dev, scaled, data)
    tr.enable_band_report(10)
    steps = tr.steps_per_epoch
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps * epochs)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rec = tr.validate(epochs - 1)
    return {"scaled": scaled, "steps": tr.global_step, "epochs": epochs, "seconds": seconds, "psnr": rec["psnr"],
            "ssim": rec["ssim"], "test_loss": rec["test_loss"], "gain": rec.get("gain"),
            "bands_err_db": [b["err_db"] for b in rec["bands"]], "bands_lo": [b["lo"] for b in rec["bands"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=200, help="back-to-back calls per timed window")
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--step-window", type=int, default=100)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "gain.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gain_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernel": kernels(dev, opts)}
    from inr_mi355x.cli import cli_fit_data
    data = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), _config(), "coil")
    res["step"] = step_times(dev, data, opts)
    res["fits"] = []
    for scaled in (False, True):
        res["fits"].append(fit(dev, scaled, data, opts.epochs))
        print(json.dumps(res["fits"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
