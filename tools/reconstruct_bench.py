"""Measures reconstruction from a checkpoint on one MI355X and writes profiles/reconstruct.json (recorded, not gated).

Per grid (the brain shape 15 x 640 x 368 and its 4x grid 15 x 2560 x 1472):
  * inr_grid_rows alone: HIP events around enough back-to-back launches to fill a good fraction of a second, after a
    warm-up; bytes = 16 per row (12 B coords + 4 B dist, written only); the rate is stated against the HBM figure of
    MI355X_MICROARCH.md (6.29 TB/s measured float4 copy, 8.0 TB/s spec);
  * the parent commit's way to the same coordinates: synthetic.create_coords on the host plus the upload (host clock
    around work that ends in a device synchronise);
  * a whole Reconstructor.render() of BASELINE config 2's network (SIREN 5 x 256, gauss 256; fresh weights: speed does not
    depend on them) in rows/s, with the peak allocated memory.

Run it under a time limit:  timeout -k 10 600 python tools/reconstruct_bench.py [--out profiles/reconstruct.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402

HBM_MEASURED_TBS = 6.29  # MI355X_MICROARCH.md: float4 copy
HBM_SPEC_TBS = 8.0
BYTES_PER_ROW = 16
MAX_CALL_ROWS = 1 << 30  # rows per inr_grid_rows call here (the entry takes < 2^31)


def time_grid_kernel(spec, dev, target_s=0.5):
    from inr_mi355x.grid import grid_rows
    n = spec.rows
    coords = torch.empty(n, 3, device=dev)
    dist = torch.empty(n, device=dev)
    cuts = list(range(0, n, MAX_CALL_ROWS)) + [n]

    def sweep():
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            grid_rows(spec, lo, hi, coords_out=coords[lo:hi], dist_out=dist[lo:hi])

    for _ in range(3):
        sweep()
    torch.cuda.synchronize()
    t0 = time.time()
    sweep()
    torch.cuda.synchronize()
    reps = max(10, min(5000, int(target_s / max(time.time() - t0, 1e-6))))
    times = []
    for _ in range(3):  # three windows: their spread is the noise
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            sweep()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    best = min(times)
    gbs = n * BYTES_PER_ROW / best / 1e9
    return {"rows": n, "bytes": n * BYTES_PER_ROW, "launches_per_sweep": len(cuts) - 1, "reps_per_window": reps,
            "seconds_per_sweep_windows": times, "seconds_per_sweep": best, "GB_per_s": gbs,
            "share_of_hbm_measured_6.29TBs": gbs / (HBM_MEASURED_TBS * 1e3),
            "share_of_hbm_spec_8.0TBs": gbs / (HBM_SPEC_TBS * 1e3), "bound": "HBM writes (16 B per row, no reads)"}


def time_host_path(C, H, W, dev, reps=3):
    from inr_mi355x.synthetic import create_coords
    make, up = [], []
    for _ in range(reps):
        t0 = time.time()
        c = create_coords(C, H, W)
        t1 = time.time()
        d = c.to(dev)
        torch.cuda.synchronize()
        t2 = time.time()
        make.append(t1 - t0)
        up.append(t2 - t1)
        del c, d
    return {"create_coords_seconds": min(make), "upload_seconds": min(up), "seconds": min(make) + min(up),
            "host_bytes": C * H * W * 12, "what": "synthetic.create_coords (torch.meshgrid of torch.linspace, CPU) + .to(device)"}


def time_render(rec, scale, dev, reps=3):
    rec.render(scale=scale)  # warm-up: workspaces, code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(reps):
        t0 = time.time()
        out = rec.render(scale=scale)
        torch.cuda.synchronize()
        times.append(time.time() - t0)
        rows = out.numel() // 2
        del out  # (the peak is one rendering's, not two)
    peak = torch.cuda.max_memory_allocated(dev)
    return {"rows": rows, "seconds_runs": times, "seconds": min(times), "rows_per_s": rows / min(times),
            "peak_allocated_bytes": peak, "output_bytes": rows * 8, "full_coordinate_tensor_would_be_bytes": rows * 12,
            "chunk_rows": rec.predict_chunk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct.json"))
    ap.add_argument("--shape", default="15,640,368")
    ap.add_argument("--scale", type=int, default=4)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reconstruct_bench needs the MI355X: nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    from inr_mi355x.grid import GridSpec
    from inr_mi355x.reconstruct import Reconstructor
    from inr_mi355x.networks import SIREN, Positional_Encoder
    C, H, W = (int(v) for v in opts.shape.split(","))
    with open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml")) as f:
        cfg = yaml.safe_load(f)
    # a checkpoint of the right layout with fresh weights
    model = SIREN(cfg["net"])
    ckpt = {"net": {k: v.detach().clone() for k, v in model.state_dict().items()},
            "enc": Positional_Encoder(cfg["encoder"], device=dev).B}
    rec = Reconstructor(cfg, ckpt, shape=(C, H, W), device=dev)
    res = {"device": torch.cuda.get_device_name(0), "shape": [C, H, W], "model": "SIREN 5 x 256, gauss 256 (configs/config_siren_kspace.yaml)",
           "grids": {}}
    for name, s in (("native", 1), ("%dx" % opts.scale, opts.scale)):
        spec = GridSpec(C, H * s, W * s)
        entry = {"grid": [C, H * s, W * s]}
        entry["grid_kernel"] = time_grid_kernel(spec, dev)
        entry["host_create_coords_plus_upload"] = time_host_path(C, H * s, W * s, dev)
        entry["grid_kernel_speedup_over_host_path"] = entry["host_create_coords_plus_upload"]["seconds"] / entry["grid_kernel"]["seconds_per_sweep"]
        entry["render"] = time_render(rec, s, dev)
        res["grids"][name] = entry
        print(json.dumps({name: entry}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": opts.out}))


if __name__ == "__main__":
    main()
