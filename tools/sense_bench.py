"""Measures SENSE-model fits on one MI355X and writes profiles/sense.json (recorded, not gated).

Kernels, at the brain shape 15 x 640 x 368, for G = 1, 4, 15 coils per call, shift = 1:
  * device time of one inr_sense_apply and one inr_sense_grad call, the method of tools/gain_bench.py: --batch calls are
    enqueued back to back through the C entry itself between ONE pair of device events and the window's time is divided by
    the batch; median of --repeats windows after --warmup.  The buffers rotate over enough copies to exceed the 256 MiB
    Infinity Cache, so every call streams from HBM;
  * bytes moved (apply: 8 + 16 G per pixel, grad: 16 + 24 G) / time as a fraction of the device-to-device copy rate (read
    + written bytes / time of a 1 GiB copy) measured in the same run the same way;
  * beside it the same math as torch complex ops with torch.fft.ifftshift copies, timed the same way (--batch calls back
    to back per window, rotating buffers) -- the baseline, not the code under test.
Step, configs/config_siren_sense.yaml on the synthetic scan: device time of each stage of one step (forwards, product
kernel, FFT, loss, inverse FFT, gradient kernel, backwards, Adam), median of --step-repeats.
Fit, one run each, same mask (grid-3*2): the SENSE-model fit for --epochs epochs (20 = the epochs of BASELINE config 2's
2840-step runs), the plain INRTrainer fit for the same epochs, and the zero-filled RSS: PSNR / SSIM and the 10-ring report.

Run it under a time limit:  timeout -k 10 900 python tools/sense_bench.py [--epochs 20] [--out FILE]
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
GROUPS = (1, 4, 15)
SCALE = 0.37


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


def raw_calls(img, sens, gx, x, dimg, dsens, G, H, W):
    from inr_mi355x import _lib as L
    lib, stream, s = L.load(), torch.cuda.current_stream().cuda_stream, ctypes.c_float(SCALE)
    a = (img.data_ptr(), sens.data_ptr(), G, H, W, s, 1, x.data_ptr(), stream)
    g = (img.data_ptr(), sens.data_ptr(), gx.data_ptr(), G, H, W, s, 1, dimg.data_ptr(), dsens.data_ptr(), stream)

    def apply():
        if lib.inr_sense_apply(*a) != 0:
            raise RuntimeError(L.last_error())

    def grad():
        if lib.inr_sense_grad(*g) != 0:
            raise RuntimeError(L.last_error())
    return apply, grad


def torch_apply(img, sens, G, H, W):
    I = torch.view_as_complex(img.view(H, W, 2))
    S = torch.view_as_complex(sens.view(G, H, W, 2))
    return torch.fft.ifftshift(SCALE * S * I[None], dim=(-2, -1))


def torch_grad(img, sens, gx, G, H, W):
    I = torch.view_as_complex(img.view(H, W, 2))
    S = torch.view_as_complex(sens.view(G, H, W, 2))
    g = torch.fft.fftshift(torch.view_as_complex(gx), dim=(-2, -1))
    return SCALE * (S.conj() * g).sum(0), SCALE * I.conj()[None] * g


def kernels(dev, opts):
    _, H, W = SHAPE
    n = H * W
    res = {"pixels": n, "shift": 1}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst
    for G in GROUPS:
        nbytes = {"apply": n * (8 + 16 * G), "grad": n * (16 + 24 * G)}
        copies = max(2, -(-(300 << 20) // nbytes["apply"]))
        sets = []
        for _ in range(copies):
            t = [torch.empty(n, 2, device=dev).normal_(0, 0.3), torch.empty(G * n, 2, device=dev).normal_(0, 0.3),
                 torch.empty(G, H, W, 2, device=dev).normal_(0, 0.3), torch.empty(G, H, W, 2, device=dev),
                 torch.empty(n, 2, device=dev), torch.empty(G * n, 2, device=dev)]
            sets.append((t, raw_calls(*t, G, H, W)))
        rec = {"coils": G, "buffer_copies_in_rotation": copies, "calls_per_window": opts.batch}
        for j, name in enumerate(("apply", "grad")):
            def window(i, j=j):
                for k in range(opts.batch):
                    sets[(i * opts.batch + k) % copies][1][j]()
            t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
            t.update(bytes=nbytes[name], bytes_per_s=nbytes[name] / (t["median_ms"] * 1e-3))
            t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
            rec[name] = t
        # the baseline the same way: --batch calls back to back between one pair of events, on rotating buffers
        def torch_window(fn, n_in):
            def window(i):
                for k in range(opts.batch):
                    fn(*sets[(i * opts.batch + k) % copies][0][:n_in], G, H, W)
            return summary([ms / opts.batch for ms in event_times(window, opts.torch_repeats, 2)])
        rec["apply"]["torch_ops"] = torch_window(torch_apply, 2)
        rec["grad"]["torch_ops"] = torch_window(torch_grad, 3)
        for name in ("apply", "grad"):
            rec[name]["torch_over_kernel"] = rec[name]["torch_ops"]["median_ms"] / rec[name]["median_ms"]
        res[f"G{G}"] = rec
        print(f"G{G}", json.dumps(rec), flush=True)
        del sets
    return res


def _config(name, **kw):
    from inr_mi355x.trainer_base import set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", name))))
    cfg.update(**kw)
    return cfg


def step_split(dev, tr, opts):
    """device milliseconds of every stage of one step on group 0, each stage timed on its own between device events"""
    from inr_mi355x.sense import sense_apply, sense_grad
    c0, c1 = tr.groups[0]
    G, H, W = c1 - c0, int(tr.shape[1]), int(tr.shape[2])
    lo, hi = c0 * tr.plane, c1 * tr.plane
    xs = tr._sens_in(lo, hi)
    m = None if tr._mask_s is None else tr._mask_s[lo:hi]
    count = max(tr._count(lo, hi), 1)
    cfg = tr.config
    st = {}

    def fwd(i):
        st["ib"] = tr.engine.forward(tr._img_in, tr.enc_B, save=True)
        st["sb"] = tr.sens_engine.forward(xs, tr.sens_enc_B, save=True)

    def app(i):
        st["x"] = sense_apply(st["ib"], st["sb"], G, H, W, tr.sense_scale, 1, out=tr._x[:G])

    def fft(i):
        st["k"] = torch.view_as_real(torch.fft.fft2(torch.view_as_complex(st["x"]), norm="ortho"))

    def loss(i):
        st["gk"] = tr.engine.loss_grad(tr.loss, st["k"].view(-1, 2), tr._gt_s[lo:hi], count, mask=m)[1]

    def ifft(i):
        st["gx"] = torch.view_as_real(torch.fft.ifft2(torch.view_as_complex(st["gk"].view(G, H, W, 2)), norm="ortho"))

    def grd(i):
        st["d"] = sense_grad(st["ib"], st["sb"], st["gx"], G, H, W, tr.sense_scale, 1)

    def bwd(i):
        fwd(i)  # a backward consumes its stash: the pair is timed and the forwards' time taken off below
        tr.engine.backward(tr._img_in, tr.enc_B, st["d"][0])
        tr.sens_engine.backward(xs, tr.sens_enc_B, st["d"][1])

    def adam(i):
        for eng in (tr.engine, tr.sens_engine):
            eng.adam_step(0.0, cfg["beta1"], cfg["beta2"], 1e-8, cfg["weight_decay"])  # lr 0: the weights stay

    out = {"coils": G}
    for name, fn in (("forwards", fwd), ("sense_apply", app), ("fft2", fft), ("loss_grad", loss), ("ifft2", ifft),
                     ("sense_grad", grd), ("forwards_plus_backwards", bwd), ("adam", adam)):
        out[name] = summary(event_times(fn, opts.step_repeats, 2))
    out["backwards_ms"] = out["forwards_plus_backwards"]["median_ms"] - out["forwards"]["median_ms"]
    ms = []
    for _ in range(opts.step_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.step(0, 0)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["whole_step_wall"] = summary(ms)
    return out


def score(tr, seconds, name):
    rec = tr.metrics()
    return {"fit": name, "steps": tr.global_step, "seconds": seconds, "psnr": rec["psnr"], "ssim": rec["ssim"],
            "sense": rec.get("sense"), "bands_err_db": [b["err_db"] for b in rec["bands"]],
            "bands_lo": [b["lo"] for b in rec["bands"]]}


def run_fit(tr, steps, name):
    tr.enable_band_report(10)
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps)
    torch.cuda.synchronize()
    return score(tr, time.time() - t0, name)


def zero_filled(tr):
    """PSNR / SSIM of the RSS of ifft2c(mask * gt) against the full data's, by the validation kernels"""
    from inr_mi355x.evalchain import ifft2c, image_metrics
    C, H, W = SHAPE
    ref = image_metrics(None, ifft2c(tr.image_full.view(C, H, W, 2)).contiguous())[0]
    m = image_metrics(ref, ifft2c(tr.image.view(C, H, W, 2)).contiguous())[1]
    psnr, ssim = m[:2].cpu().tolist()
    return {"fit": "zero_filled_rss", "psnr": psnr, "ssim": ssim}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sense.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sense_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE)}
    if not opts.skip_kernels:
        res["kernel"] = kernels(dev, opts)
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_sense import SenseFitTrainer
    cfg = _config("config_siren_sense.yaml")
    data = cli_fit_data(argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE)), cfg, "coil")
    image, coords, shape, _ = data
    tr = SenseFitTrainer(cfg, image, coords, shape, dev)
    res["step"] = step_split(dev, tr, opts)
    print("step", json.dumps(res["step"]), flush=True)
    del tr
    res["fits"] = []
    tr = SenseFitTrainer(cfg, image, coords, shape, dev)
    res["fits"].append(run_fit(tr, opts.epochs * tr.steps_per_epoch, "sense"))
    res["fits"].append(zero_filled(tr))
    del tr
    plain = {k: v for k, v in cfg.items() if k != "sense"}
    tr = INRTrainer(plain, image, coords, shape, dev)
    res["fits"].append(run_fit(tr, opts.epochs * tr.steps_per_epoch, "plain"))
    for f in res["fits"]:
        print(json.dumps(f), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
