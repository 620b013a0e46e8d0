"""Measures weighted epochs on one MI355X and writes profiles/row_sampling.json (recorded, not gated).

Kernels, at the brain shape 15 x 640 x 368 (synthetic.make_kspace) with the weights of ``row_sampling: ring-inverse``:
  * device time of inr_row_cdf and of inr_sample_epoch (coords, gt, dist and batch counts, m = n), each through the C
    entry itself with arguments built beforehand: --batch calls enqueued back to back between ONE pair of device events,
    the window's time divided by the batch; median of --repeats windows after --warmup;
  * inr_shuffle_epoch on the same buffers and the device-to-device copy rate (read + written bytes / time of a 1 GiB
    copy), measured in the same run the same way;
  * the alternative in torch on the same data: ``torch.cumsum`` of the weights, ``torch.searchsorted`` of m stratified
    thresholds, three ``index_select`` gathers -- the baseline, not the code under test.  Twice: with the thresholds in
    a random order made beforehand (``torch.randperm``, outside the timing: the same job, a permuted epoch) and in
    ascending order (rows arrive in source order -- cheaper reads, but not an epoch a fit can train from without a
    shuffle on top).
The epoch calls reuse their buffers from call to call (170 MB in all), so part of every read comes from the Infinity
Cache; the three of them are measured alike.
Fits: BASELINE config 2 (configs/config_siren_kspace.yaml, SIREN 5 x 256, batch 25 000) on the same scan with
``trajectory: spokes-92``, --steps steps (2820), ``shuffle: true`` against ``row_sampling: density``: PSNR / SSIM and the
band report of one run each.

Run it under a time limit:  timeout -k 10 900 python tools/row_sampling_bench.py [--steps 2820] [--out FILE]
"""
import argparse
import ctypes as C
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


def event_times(fn, repeats, warmup):
    """milliseconds of fn() per call, by device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def windowed(call, opts):
    def window():
        for _ in range(opts.batch):
            call()
    return dict(summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)]),
                calls_per_window=opts.batch)


def kernels(dev, opts):
    from inr_mi355x import _lib as L
    from inr_mi355x.sampling import make_weights, row_cdf
    from inr_mi355x.synthetic import make_kspace
    lib = L.load()
    Cn, H, W = SHAPE
    n = Cn * H * W
    bs = 25000
    image, coords, _ = make_kspace(Cn, H, W)
    image, coords = image.to(dev).contiguous(), coords.to(dev).contiguous()
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2).contiguous()
    w = make_weights("ring-inverse", {}, coords, image, SHAPE)
    res = {"shape": list(SHAPE), "rows": n, "batch_size": bs, "weights": "ring-inverse"}
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst

    stream = torch.cuda.current_stream().cuda_stream
    rc = row_cdf(w)
    res["total_ticks"], res["zero_weight_rows"], res["scale"] = rc.total_ticks, rc.zero_weight_rows, rc.scale
    nwords = C.c_int64(0)
    L.check(lib.inr_row_cdf_scratch(n, C.byref(nwords)))
    scratch = torch.empty(nwords.value, dtype=torch.int64, device=dev)
    cdf2 = torch.empty_like(rc.cdf)

    def checked(fn, *args):
        def call():
            if fn(*args) != 0:
                raise RuntimeError(L.last_error())
        return call

    t = windowed(checked(lib.inr_row_cdf, w.data_ptr(), None, n, C.c_double(rc.scale), cdf2.data_ptr(), scratch.data_ptr(),
                         nwords.value, stream), opts)
    assert torch.equal(cdf2, rc.cdf)
    t.update(bytes=n * (4 + 4 + 8), bytes_per_s=n * 16 / (t["median_ms"] * 1e-3))  # w twice, cdf once
    t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
    res["row_cdf"] = t
    print("row_cdf", json.dumps(t), flush=True)

    co, go, do = torch.empty_like(coords), torch.empty_like(image), torch.empty_like(dist)
    counts = torch.empty(-(-n // bs), dtype=torch.int32, device=dev)
    bufs = (coords.data_ptr(), image.data_ptr(), dist.data_ptr(), None, co.data_ptr(), go.data_ptr(), do.data_ptr(), None,
            counts.data_ptr(), None, stream)
    row_bytes = 2 * (12 + 8 + 4)
    for name, call in (("sample_epoch", checked(lib.inr_sample_epoch, rc.cdf.data_ptr(), n, n, bs, C.c_uint64(1),
                                                C.c_uint32(3), *bufs)),
                       ("shuffle_epoch", checked(lib.inr_shuffle_epoch, n, bs, C.c_uint64(1), C.c_uint32(3), *bufs))):
        t = windowed(call, opts)
        t.update(gathered_bytes=n * row_bytes, gathered_bytes_per_s=n * row_bytes / (t["median_ms"] * 1e-3))
        t["fraction_of_copy_rate"] = t["gathered_bytes_per_s"] / copy_rate
        res[name] = t
        print(name, json.dumps(t), flush=True)

    wd = w.double()

    def torch_cdf():
        return torch.cumsum(wd, 0)

    tcdf = torch_cdf()
    u_sorted = (torch.arange(n, device=dev, dtype=torch.float64) + 0.5) * (float(tcdf[-1]) / n)
    u_permuted = u_sorted[torch.randperm(n, device=dev)].contiguous()

    def torch_draw(u):
        idx = torch.searchsorted(tcdf, u, right=True).clamp_(max=n - 1)
        return coords.index_select(0, idx), image.index_select(0, idx), dist.index_select(0, idx)

    res["torch_cumsum"] = summary(event_times(torch_cdf, opts.torch_repeats, 2))
    res["torch_searchsorted_index_select"] = summary(event_times(lambda: torch_draw(u_permuted), opts.torch_repeats, 2))
    res["torch_searchsorted_index_select_sorted"] = summary(event_times(lambda: torch_draw(u_sorted), opts.torch_repeats, 2))
    res["ratios"] = {
        "sample_over_shuffle": res["sample_epoch"]["median_ms"] / res["shuffle_epoch"]["median_ms"],
        "torch_draw_over_sample": res["torch_searchsorted_index_select"]["median_ms"] / res["sample_epoch"]["median_ms"],
        "torch_sorted_draw_over_sample": res["torch_searchsorted_index_select_sorted"]["median_ms"]
        / res["sample_epoch"]["median_ms"],
        "torch_cumsum_over_row_cdf": res["torch_cumsum"]["median_ms"] / res["row_cdf"]["median_ms"],
    }
    print("ratios", json.dumps(res["ratios"]), flush=True)
    return res


def fit(dev, extra, steps):
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.train import INRTrainer, set_default_configs
    cfg = set_default_configs(yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))))
    cfg.update(undersampling=None, trajectory="spokes-92", **extra)
    opts = argparse.Namespace(synthetic=",".join(str(v) for v in SHAPE))
    image, coords, shape, cc = cli_fit_data(opts, cfg, "coil")
    tr = INRTrainer(cfg, image, coords, shape, dev, coil_compression=cc)
    tr.enable_band_report(10)
    torch.cuda.synchronize()
    t0 = time.time()
    tr.fit(steps)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rec = tr.validate(tr.global_step // tr.steps_per_epoch)
    return dict(extra, trajectory="spokes-92", steps=tr.global_step, steps_per_epoch=tr.steps_per_epoch, seconds=seconds,
                psnr=rec["psnr"], ssim=rec["ssim"], row_sampling_record=rec.get("row_sampling"),
                bands_err_db=[b["err_db"] for b in rec["bands"]], bands_lo=[b["lo"] for b in rec["bands"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2820)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--torch-repeats", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "row_sampling.json"))
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("row_sampling_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernels(dev, opts), "fits": []}
    for extra in (dict(shuffle=True), dict(row_sampling="density")):
        res["fits"].append(fit(dev, extra, opts.steps))
        print(json.dumps(res["fits"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
