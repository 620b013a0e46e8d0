"""Measures the Kaiser-Bessel gridding operator pair (csrc/inr_nufft.hip) on one MI355X and writes
profiles/nufft.json (recorded, not gated).

At the brain shape 15 x 640 x 368 (synthetic.make_kspace), for spokes-92 and spokes-1005 in the same run: HIP events around
back-to-back calls after a warm-up, three windows, the median reported with all three listed --
  trajectory.nufft and nufft_adjoint (scratch, bins and apodisation made beforehand; torch.fft included);
  the four library calls on their own (prepare, interp, spread, finish), the two HBM-bound ones (prepare, finish) with
  the bytes they must move and the share that is of the copy rate measured first in this run (a 1 GiB device copy);
  the exact pair inr_nudft / inr_adjoint_nudft (at spokes-1005 only if its tables fit in free memory: said either way);
  trajectory.cg_baseline with 10 iterations under both operators (wall clock around a synchronised call).
Quality: PSNR / SSIM / objective of cg-10 under both operators on BASELINE config 2's synthetic scan, spokes-92.

Run it under a time limit:  timeout -k 10 900 python tools/nufft_bench.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402

from nudft_bench import SHAPE, windows  # noqa: E402


def copy_rate(dev):
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty_like(a)
    r = windows(lambda: b.copy_(a), reps=10)
    r["bytes_per_second"] = 2 * a.numel() * 4 / r["seconds"]
    return r


def timed_cg(T, val, pos, w, operator):
    def run():
        torch.cuda.synchronize()
        t0 = time.time()
        iterates, objective = T.cg_baseline(val, pos, SHAPE, w, 10, operator=operator)
        torch.cuda.synchronize()
        return time.time() - t0, iterates[-1], objective

    run()
    runs = [run() for _ in range(3)]
    return {"iters": 10, "seconds_runs": [r[0] for r in runs], "seconds": sorted(r[0] for r in runs)[1],
            "objective": runs[0][2]}, runs[0][1]


def measure(dev, img, ref_rss, n_spokes, rate):
    from inr_mi355x import _lib as L
    from inr_mi355x import trajectory as T
    from inr_mi355x.evalchain import image_metrics
    C, H, W = SHAPE
    pos_np = T.spokes(H, W, n_spokes)
    M = pos_np.shape[0]
    pos = torch.from_numpy(pos_np).to(dev)
    w_np = T.density_ramp(n_spokes, M // n_spokes, H, W)
    w = torch.from_numpy(w_np).float().to(dev)
    res = {"trajectory": "spokes-%d" % n_spokes, "rows_per_coil": M}
    taps = torch.empty(T.nufft_scratch_floats(C, H, W, M), device=dev)
    t0 = time.time()
    bins = T.nufft_device_bins(pos_np, H, W, dev)
    res["nufft_bins_host_seconds"] = time.time() - t0
    apod = T.nufft_device_apodisation(H, W, dev)
    val = T.nufft(img, pos, scratch=taps, apod=apod)
    res["gridding_forward"] = windows(lambda: T.nufft(img, pos, scratch=taps, apod=apod), reps=10)
    res["gridding_adjoint"] = windows(lambda: T.nufft_adjoint(val, pos, (H, W), w, scratch=taps, bins=bins, apod=apod), reps=10)
    lib, st = L.load(), torch.cuda.current_stream(dev).cuda_stream
    grid = torch.zeros(C, 2 * H, 2 * W, 2, device=dev)
    out = torch.empty(C, H, W, 2, device=dev)
    image_bytes = C * H * W * 8
    passes = {
        "prepare": (lambda: L.check(lib.inr_nufft_prepare(img.data_ptr(), apod[0].data_ptr(), apod[1].data_ptr(), C, H, W,
                                                          grid.data_ptr(), st)), 5 * image_bytes),
        "interp": (lambda: L.check(lib.inr_nufft_interp(grid.data_ptr(), pos.data_ptr(), C, H, W, M, val.data_ptr(),
                                                        taps.data_ptr(), taps.numel(), st)), None),
        "spread": (lambda: L.check(lib.inr_nufft_spread(val.data_ptr(), pos.data_ptr(), w.data_ptr(), bins[0].data_ptr(),
                                                        bins[1].data_ptr(), C, H, W, M, grid.data_ptr(), taps.data_ptr(),
                                                        taps.numel(), st)), None),
        "finish": (lambda: L.check(lib.inr_nufft_finish(grid.data_ptr(), apod[0].data_ptr(), apod[1].data_ptr(), C, H, W,
                                                        out.data_ptr(), st)), 2 * image_bytes),
    }
    val_keep = val.clone()
    for name, (fn, nbytes) in passes.items():
        r = windows(fn, reps=10)
        if nbytes is not None:
            r.update(bytes=nbytes, share_of_copy_rate=nbytes / r["seconds"] / rate)
        res[name] = r
    val.copy_(val_keep)
    del grid, out
    torch.cuda.empty_cache()
    need = 4 * (T.scratch_floats(C, H, W, M) + T.adjoint_scratch_floats(C, H, W, M))
    free = torch.cuda.mem_get_info(dev)[0]
    res["exact_scratch_bytes"], res["exact_scratch_fits"] = need, bool(need < free // 2)
    if res["exact_scratch_fits"]:
        fs = torch.empty(T.scratch_floats(C, H, W, M), device=dev)
        ads = torch.empty(T.adjoint_scratch_floats(C, H, W, M), device=dev)
        res["exact_forward"] = windows(lambda: T.nudft(img, pos, scratch=fs), reps=2)
        res["exact_adjoint"] = windows(lambda: T.nudft_adjoint(val, pos, (H, W), w, scratch=ads), reps=2)
        del fs, ads
        torch.cuda.empty_cache()
        y = T.nudft(img, pos)  # the samples a fit would train on
    else:
        y = val
    for operator in ("gridding", "exact") if res["exact_scratch_fits"] else ("gridding",):
        rec, image = timed_cg(T, y, pos, w_np, operator)
        m = image_metrics(ref_rss, image.contiguous())[1][:2].cpu().tolist()
        rec.update(psnr=m[0], ssim=m[1])
        res["cg_10_" + operator] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nufft.json"))
    opts = ap.parse_args()
    from inr_mi355x.evalchain import ifft2c, image_metrics
    from inr_mi355x.synthetic import make_kspace
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml")))
    C, H, W = SHAPE
    k = make_kspace(C, H, W, normalization=cfg["normalization"])[0].reshape(C, H, W, 2).to(dev)
    img = ifft2c(k).contiguous()
    ref_rss = image_metrics(None, img)[0]
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "copy": copy_rate(dev)}
    print(json.dumps(res["copy"]), flush=True)
    for n_spokes in (92, 1005):
        res["spokes-%d" % n_spokes] = measure(dev, img, ref_rss, n_spokes, res["copy"]["bytes_per_second"])
        print(json.dumps(res["spokes-%d" % n_spokes]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
