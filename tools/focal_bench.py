"""Measures the focal frequency loss (``loss: FFL``) on one MI355X and writes profiles/focal.json (recorded, not gated;
DESIGN.md 4.26).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace) and at 25 000 rows, defaults (alpha 1, log matrix), with
dout:
  * device time of one inr_focal_loss_grad call (three launches), the method of tools/gain_bench.py: --batch calls are
    enqueued back to back through the C entry itself (arguments built beforehand) between ONE pair of device events and the
    window's time is divided by the batch; median of --repeats windows after --warmup.  The buffers rotate over enough
    copies to exceed the 256 MiB Infinity Cache, so every call streams from HBM.  Where the host enqueues more slowly than
    the device runs (the 25 000-row case) it is an upper bound;
  * its 40 bytes per row / time (out and gt read twice, dout written once) as a fraction of the device-to-device copy rate
    (read + written bytes / time of a 1 GiB copy) measured in the same run the same way;
  * beside it the reference's formula in torch ops on the same resident tensors (the weight detached, autograd to out) --
    the baseline, not the code under test.
Step, BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan: wall time per step
of an FFL fit against the same tree's L2 fit as tier-1 calls (INR_ONE_CALL_STEPS=0: the same launches but for the loss) and
as its default one-call step: what the tier-1 route costs.
Fit: the same config under FFL against L2, same steps and seed: PSNR / SSIM of validate() and its 10-ring band report after
--epochs epochs (20 epochs = 2840 steps), ONE run each.

Run it under a time limit:  timeout -k 10 900 python tools/focal_bench.py [--epochs 20] [--out FILE]
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
BYTES_PER_ROW = 40  # pass 1: out 8, gt 8 read; pass 2: out 8, gt 8 read, dout 8 written; no mask (+2)


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


def raw_call(d, out, gt, loss, dout):
    from inr_mi355x import _lib as L
    fn, stream = L.load().inr_focal_loss_grad, torch.cuda.current_stream().cuda_stream
    args = (ctypes.byref(d), out.data_ptr(), gt.data_ptr(), None, out.shape[0], loss.data_ptr(), dout.data_ptr(), stream)

    def call(keep=d):
        if fn(*args) != 0:
            raise RuntimeError(L.last_error())
    return call


def torch_way(out, gt):
    """FocalFrequencyLoss.loss_formulation (matrix = None, defaults) in torch ops, and its gradient"""
    out = out.detach().requires_grad_(True)
    tmp = (out - gt) ** 2
    m = torch.log(torch.sqrt(tmp[..., 0] + tmp[..., 1]) + 1.0)
    m = m / m.max()
    m[torch.isnan(m)] = 0.0
    w = torch.clamp(m, min=0.0, max=1.0).clone().detach()
    tmp = (out - gt) ** 2
    loss = torch.mean(w * (tmp[..., 0] + tmp[..., 1]))
    return (loss,) + torch.autograd.grad(loss, (out,))


def kernels(dev, opts):
    from inr_mi355x import _lib as L
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    image = make_kspace(C, H, W)[0].to(dev).contiguous()
    res = {"bytes_per_row": BYTES_PER_ROW, "alpha": 1.0, "log_matrix": True, "blocks": L.FOCAL_BLOCKS, "launches": 3}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    for name, n in (("brain", C * H * W), ("rows25000", 25000)):
        gt = image[:n].contiguous()
        copies = max(2, -(-(300 << 20) // (n * 24)))  # 24 distinct bytes per row and set
        d = L.FocalDesc(alpha=1.0, log_matrix=1, loss_weight=1.0, inv_count=1.0 / n)
        sets = []
        for _ in range(copies):
            y = torch.empty(n, 2, device=dev).normal_(0, 0.3)
            sets.append((y, gt.clone(), torch.zeros(L.LOSS_WORDS, device=dev), torch.empty_like(y)))
        calls = [raw_call(d, *st) for st in sets]

        def window(i, calls=calls, copies=copies):
            for k in range(opts.batch):
                calls[(i * opts.batch + k) % copies]()
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(rows=n, calls_per_window=opts.batch, buffer_copies_in_rotation=copies, bytes=n * BYTES_PER_ROW,
                 bytes_per_s=n * BYTES_PER_ROW / (t["median_ms"] * 1e-3))
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        y, g = sets[0][0], sets[0][1]
        tw = summary(event_times(lambda i: torch_way(y, g), opts.torch_repeats, 2))
        t["torch_ops"] = tw
        t["torch_over_kernel"] = tw["median_ms"] / t["median_ms"]
        # the two ways agree on what they compute (a check of the baseline, not a parity test)
        calls[0]()
        loss_t, grad_t = torch_way(y, g)
        t["loss_kernel"], t["loss_torch_ops"] = float(sets[0][2][0]), float(loss_t)
        t["grad_rel_l2_vs_torch_ops"] = float((sets[0][3] - grad_t).norm() / grad_t.norm())
        res[name] = t
        print(name, json.dumps(t), flush=True)
        del sets, calls
    return res


def _config(loss):
    from inr_mi355x.trainer_base import set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(undersampling=None, loss=loss)
    return cfg


def _trainer(dev, loss, data, one_call=True):
    from inr_mi355x.train import INRTrainer
    image, coords, shape, cc = data
    old = os.environ.get("INR_ONE_CALL_STEPS")
    os.environ["INR_ONE_CALL_STEPS"] = "1" if one_call else "0"  # read by the constructor
    try:
        return INRTrainer(_config(loss), image, coords, shape, dev, coil_compression=cc)
    finally:
        if old is None:
            del os.environ["INR_ONE_CALL_STEPS"]
        else:
            os.environ["INR_ONE_CALL_STEPS"] = old


def step_times(dev, data, opts):
    """wall milliseconds per step over windows of --step-window steps of epoch 0 (full batches of 25 000 rows)"""
    out = {}
    for name, loss, one_call in (("ffl_tier1", "FFL", True), ("l2_tier1_two_calls", "L2", False),
                                 ("l2_fused_one_call", "L2", True)):
        tr = _trainer(dev, loss, data, one_call)
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
        out[name] = dict(summary(ms), steps_per_window=n, batch=tr.bs, one_call_steps=bool(tr.one_call_steps))
        print(name, json.dumps(out[name]), flush=True)
        del tr
    out["ffl_over_l2_tier1"] = out["ffl_tier1"]["median_ms"] / out["l2_tier1_two_calls"]["median_ms"]
    out["ffl_over_l2_fused"] = out["ffl_tier1"]["median_ms"] / out["l2_fused_one_call"]["median_ms"]
    return out


def fit(dev, loss, data, epochs):
    tr = _trainer(dev, loss, data)
    tr.enable_band_report(10)
    steps = tr.steps_per_epoch
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps * epochs)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rec = tr.validate(epochs - 1)
    return {"loss": loss, "steps": tr.global_step, "epochs": epochs, "seconds": seconds, "psnr": rec["psnr"],
            "ssim": rec["ssim"], "test_loss": rec["test_loss"], "focal": rec.get("focal"), "runs": 1,
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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "focal.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focal_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernel": kernels(dev, opts)}
    from inr_mi355x.cli import cli_fit_data
    data = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), _config("L2"), "coil")
    res["step"] = step_times(dev, data, opts)
    res["fits"] = []
    for loss in ("L2", "FFL"):
        res["fits"].append(fit(dev, loss, data, opts.epochs))
        print(json.dumps(res["fits"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
