"""Measures the radial band statistics kernel (inr_band_stats) on the brain shape and writes
profiles/band_stats.json:

  * device time of one inr_band_stats call (both launches), for the 40 rings and for the 4 partitions of the k-means
    split, without and with a prediction: --batch calls are enqueued back to back through the C entry itself (arguments
    built beforehand, so the host spends a ctypes call and two launches per call) between ONE pair of device events,
    and the window's time is divided by the batch; median of --repeats windows after --warmup.  The inputs rotate over
    enough copies to exceed the 256 MiB Infinity Cache, so every call streams from HBM.  It is device time per call
    at a full queue, not a profiler's kernel time: where the host enqueues more slowly than the device runs, it is an
    upper bound;
  * its input bytes / time as a fraction of the device-to-device copy rate (read + written bytes / time of a 1 GiB
    copy) measured in the same run the same way;
  * wall time of partition_kspace + partition_and_stats on device tensors, this commit against the parent commit's
    clustering.py (--parent FILE: `git show <parent>:mri-implicit-neural-representations_amd/inr_mi355x/clustering.py`),
    alternating, each ended by a device synchronise; and that labels, radii and stats agree.

    python tools/band_stats_bench.py [--shape 15,640,368] [--parent FILE] [--out profiles/band_stats.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mri-implicit-neural-representations_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def raw_call(dist, gt, pred, bounds):
    """() -> one inr_band_stats call on the current stream, every argument prepared here"""
    import ctypes as C
    from inr_mi355x import _lib as L
    from inr_mi355x import bands
    lo, hi, _ = bands.band_stats_device(dist, gt, pred, bounds=bounds)  # checks, and the cached stats / scratch buffers
    stats, scratch = bands._scratch[(dist.numel(), len(lo), dist.device)]
    FP = C.POINTER(C.c_float)
    fn, stream = L.load().inr_band_stats, torch.cuda.current_stream().cuda_stream
    args = (dist.data_ptr(), gt.data_ptr(), None if pred is None else pred.data_ptr(), None, 1, dist.numel(),
            lo.ctypes.data_as(FP), hi.ctypes.data_as(FP), len(lo), stats.data_ptr(), scratch.data_ptr(), stream)

    def call(keep=(lo, hi, stats, scratch)):
        if fn(*args) != 0:
            raise RuntimeError(L.last_error())
    return call


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=str, default="15,640,368")
    ap.add_argument("--parent", type=str, default=None, help="the parent commit's clustering.py")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "band_stats.json"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--wall-repeats", type=int, default=5)
    opts = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("band_stats_bench: no GPU (a CPU run measures nothing)")
    from inr_mi355x import bands, clustering
    from inr_mi355x.synthetic import make_kspace
    dev = torch.device("cuda:0")
    C, H, W = (int(v) for v in opts.shape.split(","))
    image, coords, _ = make_kspace(C, H, W)
    n = C * H * W
    img, kc = image.to(dev).reshape(C, H, W, 2), coords.to(dev).reshape(C, H, W, 3)
    res = {"device": torch.cuda.get_device_name(0), "shape": [C, H, W], "rows": n}

    # the copy rate, same method
    words = (1 << 30) // 4
    src, dst = torch.empty(words, device=dev).normal_(), torch.empty(words, device=dev)
    copy = summary(event_times(lambda i: dst.copy_(src), opts.repeats, opts.warmup))
    copy_rate = 2.0 * words * 4 / (copy["median_ms"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * words * 4, bytes_per_s=copy_rate)
    del src, dst

    dist = torch.sqrt(kc[..., 1] ** 2 + kc[..., 2] ** 2).reshape(-1).contiguous()
    gt = img.reshape(-1, 2).contiguous()
    pred = gt + 0.01 * torch.randn_like(gt)
    _, radii = clustering.partition_kspace(img, kc, 40, 4)
    cases = {"rings40": bands.ring_bounds(40), "parts4": [(float(radii[i]), float(radii[i + 1])) for i in range(4)]}
    copies = max(2, -(-(300 << 20) // (n * 12)))  # > 256 MiB of inputs in rotation even without pred
    sets = [(dist.clone(), gt.clone(), pred.clone()) for _ in range(copies)]
    res["input_copies_in_rotation"] = copies
    res["kernel"] = {}
    for name, bounds in cases.items():
        for with_pred in (False, True):
            calls = [raw_call(d, g, p if with_pred else None, bounds) for d, g, p in sets]

            def window(i, calls=calls):
                for k in range(opts.batch):
                    calls[(i * opts.batch + k) % copies]()
            t = summary([ms / opts.batch for ms in event_times(window, opts.repeats, opts.warmup)])
            t["calls_per_window"] = opts.batch
            nbytes = n * (12 + (8 if with_pred else 0))
            t.update(bands=len(bounds), input_bytes=nbytes, bytes_per_s=nbytes / (t["median_ms"] * 1e-3))
            t["fraction_of_copy_rate"] = t["bytes_per_s"] / copy_rate
            res["kernel"][name + ("_pred" if with_pred else "")] = t
    del sets

    # wall time of the partition, this commit against the parent's loop
    def wall(mod):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels, r = mod.partition_kspace(img, kc, 40, 4)
        stats, r2 = mod.partition_and_stats(img, kc, 40, 4)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, (np.asarray(labels), np.asarray(r), stats.cpu().numpy(), np.asarray(r2))

    mods = {"this_commit": clustering}
    if opts.parent:
        spec = importlib.util.spec_from_file_location("parent_clustering", opts.parent)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        mods["parent_commit"] = parent
    times, outs = {k: [] for k in mods}, {}
    for rep in range(opts.wall_repeats + 1):  # the first round warms both up
        for k, mod in mods.items():
            t, outs[k] = wall(mod)
            if rep:
                times[k].append(t)
    res["partition_wall"] = {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "repeats": len(v)}
                             for k, v in times.items()}
    if "parent_commit" in outs:
        a, b = outs["this_commit"], outs["parent_commit"]
        res["partition_wall"]["same_labels_radii"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        res["partition_wall"]["same_stats"] = bool(np.array_equal(a[2], b[2]))
        res["partition_wall"]["speedup"] = (res["partition_wall"]["parent_commit"]["median_s"]
                                            / res["partition_wall"]["this_commit"]["median_s"])
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
