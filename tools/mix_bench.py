"""Measures mixture-of-heads fits on one MI355X and writes profiles/mix.json (recorded, not gated).

Kernel, at the brain shape 15 x 640 x 368 (synthetic.make_kspace), L2 loss, with res, for K = 2, 4, 8:
  * device time of one inr_mix_loss_grad call, the method of tools/gain_bench.py: --batch calls are enqueued back to back
    through the C entry itself (arguments built beforehand) between ONE pair of device events and the window's time is
    divided by the batch; median of --repeats windows after --warmup.  The buffers rotate over enough copies to exceed the
    256 MiB Infinity Cache, so every call streams from HBM;
  * its 8 (2K + 2) + 8K + 4 bytes per row / time as a fraction of the device-to-device copy rate (read + written bytes /
    time of a 1 GiB copy) measured in the same run the same way;
  * beside it the torch-op restatement on the same resident tensors (the mix, the clamp, 0.5 MSE on the mix and per ring,
    autograd to every y_k and to w) -- the baseline, not the code under test.
Step, BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan: wall time per
step of MixtureFitTrainer (K = 4) against the same network's INRTrainer.
Fit: K = 4 mixture with detach true and false, the plain fit and the 4-ring ensemble, same seed, --steps steps each
(2840 = 20 epochs): PSNR / SSIM of metrics() and its 10-ring band report, one run each.

Run it under a time limit:  timeout -k 10 900 python tools/mix_bench.py [--steps 2840] [--out FILE]
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
HEADS = (2, 4, 8)


def bytes_per_row(K):
    return 8 * (2 * K + 2) + 8 * K + 4  # y_k, gt read, dy_k, res written; w read, dw written; dist read; no mask (+1)


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


def raw_call(ld, desc, w, gt, dist, res, loss, dw):
    from inr_mi355x import _lib as L
    fn, stream = L.load().inr_mix_loss_grad, torch.cuda.current_stream().cuda_stream
    args = (ctypes.byref(ld), ctypes.byref(desc), w.data_ptr(), gt.data_ptr(), dist.data_ptr(), None, w.shape[0],
            res.data_ptr(), loss.data_ptr(), dw.data_ptr(), stream)

    def call(keep=(ld, desc)):
        if fn(*args) != 0:
            raise RuntimeError(L.last_error())
    return call


def torch_way(ys, w, gt, rings, inv):
    ys = [y.detach().requires_grad_(True) for y in ys]
    w = w.detach().requires_grad_(True)
    pre = sum(w[:, k:k + 1] * y.detach() for k, y in enumerate(ys))
    loss = 0.5 * torch.nn.functional.mse_loss(torch.clamp(pre, -1.0, 1.0), gt)
    for k, y in enumerate(ys):
        e = (y - gt) * rings[k][:, None]
        loss = loss + 0.25 * inv[1 + k] * (e * e).sum()
    return torch.autograd.grad(loss, ys + [w])


def kernels(dev, opts):
    from inr_mi355x import _lib as L
    from inr_mi355x import mix as M
    from inr_mi355x.gain import gain_inputs
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    C, H, W = SHAPE
    n = C * H * W
    gt = make_kspace(C, H, W)[0].to(dev).contiguous()
    dist = gain_inputs(grid_coords(C, H, W, device=dev))[:, 1].contiguous()
    res = {"loss": "L2", "blocks": L.MIX_BLOCKS, "rows": n}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    for K in HEADS:
        radii = [float(torch.tensor(1.4143 * k / K, dtype=torch.float32)) for k in range(K + 1)]
        inv = M.inv_counts(M.ring_counts(dist, None, radii))
        bpr = bytes_per_row(K)
        copies = max(2, -(-(300 << 20) // (n * bpr)))
        ld = L.LossDesc(kind=L.LOSS_L2_HALF, eps=1e-3, sigma=2.0, factor=0.5, inv_count=inv[0], hdr_A=0.0)
        sets, calls = [], []
        for _ in range(copies):
            ys = [torch.empty(n, 2, device=dev).normal_(0, 0.3) for _ in range(K)]
            w = torch.empty(n, K, device=dev).uniform_(0, 1)
            dys = [torch.empty_like(y) for y in ys]
            bufs = (w, gt.clone(), dist.clone(), torch.empty(n, 2, device=dev), torch.zeros(L.LOSS_WORDS, device=dev),
                    torch.empty_like(w))
            desc = M._desc(ys, dys, radii, inv, True, True)
            sets.append((ys, dys, bufs))
            calls.append(raw_call(ld, desc, *bufs))

        def window(i, calls=calls, copies=copies):
            for k in range(opts.batch):
                calls[(i * opts.batch + k) % copies]()
        t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
        t.update(heads=K, bytes_per_row=bpr, calls_per_window=opts.batch, buffer_copies_in_rotation=copies, bytes=n * bpr,
                 bytes_per_s=n * bpr / (t["median_ms"] * 1e-3))
        t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
        ys, w, g = sets[0][0], sets[0][2][0], sets[0][2][1]
        rings = [((dist >= radii[k]) & (dist <= radii[k + 1])).float() for k in range(K)]
        tw = summary(event_times(lambda i: torch_way(ys, w, g, rings, inv), opts.torch_repeats, 2))
        t["torch_ops"] = tw
        t["torch_over_kernel"] = tw["median_ms"] / t["median_ms"]
        res[f"K{K}"] = t
        print(f"K{K}", json.dumps(t), flush=True)
        del sets, calls, rings
    return res


def _config(name="config_siren_kspace.yaml", **kw):
    from inr_mi355x.trainer_base import set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", name))))
    cfg.update(undersampling=None, **kw)
    return cfg


def _trainer(dev, which, data):
    image, coords, shape, cc = data
    if which == "plain":
        from inr_mi355x.train import INRTrainer
        return INRTrainer(_config(), image, coords, shape, dev, coil_compression=cc)
    if which == "ensemble":
        from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
        return RingEnsembleTrainer(_config(partition={"no_steps": 40, "no_models": 4}), image, coords, shape, dev,
                                   coil_compression=cc)
    from inr_mi355x.train_multihead import MixtureFitTrainer
    cfg = _config("config_siren_multihead.yaml")
    cfg["mixture"] = dict(cfg["mixture"], detach=which == "mixture_detach")
    return MixtureFitTrainer(cfg, image, coords, shape, dev, coil_compression=cc)


def step_times(dev, data, opts):
    """wall milliseconds per step over windows of --step-window steps of epoch 0 (full batches of 25 000 rows)"""
    out = {}
    for name in ("mixture_detach", "plain"):
        tr = _trainer(dev, name, data)
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
    out["mixture_over_plain"] = out["mixture_detach"]["median_ms"] / out["plain"]["median_ms"]
    return out


def fit(dev, which, data, steps):
    tr = _trainer(dev, which, data)
    tr.enable_band_report(10)
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rec = tr.metrics()
    out = {"fit": which, "steps": tr.global_step, "seconds": seconds, "psnr": rec["psnr"], "ssim": rec["ssim"],
           "mixture": rec.get("mixture"), "radii": getattr(tr, "radii", None),
           "bands_err_db": [b["err_db"] for b in rec["bands"]], "bands_lo": [b["lo"] for b in rec["bands"]]}
    if which.startswith("mixture"):
        out["loss_terms_last_step"] = tr.loss_terms()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2840)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--step-window", type=int, default=100)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mix.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernel": kernels(dev, opts)}
    from inr_mi355x.cli import cli_fit_data
    data = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), _config(), "coil")
    res["step"] = step_times(dev, data, opts)
    res["fits"] = []
    for which in ("mixture_detach", "mixture_joint", "plain", "ensemble"):
        res["fits"].append(fit(dev, which, data, opts.steps))
        print(json.dumps(res["fits"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
