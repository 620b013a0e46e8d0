"""Measurement (GPU): the headline workload (bench.CONFIG: SIREN 5x256, gauss-512, batch 25 000, synthetic 15 x 640 x 368,
fp32) fitted with sequential and with shuffled epochs (config['shuffle']), in one process on one box.

Writes a JSON file (default profiles/shuffle_fit.json) with
  (a) PSNR at 1 000 steps and after 10 epochs for both orders: the mean over the last full epoch's reads, taken at the
      SAME step numbers in both runs (bench.psnr_read_steps: the sequential sweep's end-of-coil steps -- they mean
      nothing in a shuffled epoch, so the file names them);
  (b) the median per-step time from HIP events for sequential, sequential again (the A/A spread) and shuffled, the three
      trainers alive together and taking turns epoch by epoch;
  (c) the time of one inr_shuffle_epoch call (HIP events) and its bytes against the figures derived in DESIGN.md 4.12;
  (d) the wall time of an epoch boundary (kernel + the read-back of the batch counts), as a share of the epoch and
      against the host route (torch.randperm + mask gather + cumulative sum, measured on a CPU: 0.43 s).

    python tools/shuffle_fit.py [--out FILE] [--epochs 10] [--time-rounds 6]"""
import argparse
import json
import os
import socket
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mri-implicit-neural-representations_amd"))
import torch
import bench
from inr_mi355x.shuffle import shuffle_epoch
from inr_mi355x.synthetic import make_kspace
from inr_mi355x.train import INRTrainer

HOST_ROUTE_S = 0.43  # torch.randperm of 15 x 640 x 368 rows (0.24 s) + mask gather and cumulative sum (0.19 s), CPU, torch 2.10
LINE = 64            # bytes of one cache line: what a single-row read can pull at worst


def kernel_bytes(n: int) -> dict:
    """DESIGN.md 4.12 for the headline fit (coords + image, no mask, no dist): every row is read once and written once
    (`useful`); a row read alone in its line pulls the whole line, a 12-byte row straddles two lines in 2 of 16
    positions (`worst`, what the memory side moves if no line is ever shared between two reads)."""
    useful = n * (12 + 8) * 2
    worst = n * (LINE * (1 + 2 / 16) + LINE) + n * (12 + 8)
    return {"useful": useful, "worst_case_line_amplified": int(worst)}


def psnr_runs(cfg, image, coords, shape, dev, epochs):
    out, steps = {}, {}
    for name, c in (("sequential", cfg), ("shuffled", dict(cfg, shuffle=True))):
        tr = INRTrainer(c, image, coords, shape, dev, seed=0)
        spe = tr.steps_per_epoch
        totals = [1000, epochs * spe]
        reads, at = set(), {}
        for t in totals:
            r, at[t] = bench.psnr_read_steps(t, spe, tr.bs, bench.SHAPE[1] * bench.SHAPE[2], bench.SHAPE[0])
            reads |= set(r)
        got = bench.fit_with_reads(tr, 0, max(totals), reads)
        print(f"{name}: {len(got)} PSNR reads over {max(totals)} steps", flush=True)
        out[name] = {str(t): bench.psnr_summary({k: got[k] for k in got if k <= t}, at[t]) for t in totals}
        for t in totals:
            out[name][str(t)]["single_read_db"] = got[t]
        steps = {str(t): at[t] for t in totals}
        del tr
    for t in steps:
        out["shuffled_minus_sequential_db_" + t] = out["shuffled"][t]["mean_db"] - out["sequential"][t]["mean_db"]
    out["read_steps"] = steps
    return out


def step_times(cfg, image, coords, shape, dev, rounds):
    """Per-step HIP-event times, epoch by epoch in turns; a shuffled epoch's refill runs before its first timed step and is
    timed on its own with a host clock around it (it ends in the read-back of the counts, which synchronises)."""
    trs = {"sequential_a": INRTrainer(cfg, image, coords, shape, dev, seed=0),
           "sequential_b": INRTrainer(cfg, image, coords, shape, dev, seed=0),
           "shuffled": INRTrainer(dict(cfg, shuffle=True), image, coords, shape, dev, seed=0)}
    spe = trs["shuffled"].steps_per_epoch
    ms = {k: [] for k in trs}
    boundary = []
    for epoch in range(rounds + 1):  # epoch 0 warms every shape up (full batches and the short last one)
        for name, tr in trs.items():
            if tr.shuffle:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr._begin_shuffled(epoch, 0)
                boundary.append(time.perf_counter() - t0)
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(spe + 1)]
            evs[0].record()
            for it in range(spe):
                tr.step(epoch, it)
                evs[it + 1].record()
            torch.cuda.synchronize()
            if epoch > 0:
                ms[name] += [evs[i].elapsed_time(evs[i + 1]) for i in range(spe - 1)]  # full batches only
    med = {k: st.median(v) for k, v in ms.items()}
    aa = abs(med["sequential_a"] - med["sequential_b"])
    seq = 0.5 * (med["sequential_a"] + med["sequential_b"])
    b = st.median(boundary[1:])
    return {"median_step_ms": med, "steps_timed_each": len(ms["shuffled"]), "aa_spread_ms": aa,
            "shuffled_minus_sequential_ms": med["shuffled"] - seq,
            "shuffled_within_aa_spread": abs(med["shuffled"] - seq) <= max(aa, 0.0) + 1e-12,
            "epoch_boundary": {"wall_ms_median": 1e3 * b, "wall_ms_all": [1e3 * x for x in boundary],
                               "share_of_epoch": b / (b + 1e-3 * spe * med["shuffled"]),
                               "host_route_s": HOST_ROUTE_S, "host_route_over_boundary": HOST_ROUTE_S / b}}, trs["shuffled"]


def kernel_time(tr, dev, reps=20):
    eb = tr._epoch_buf
    coords, image, _, _ = eb.src
    ms = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        shuffle_epoch(eb.n, 0, 100 + r, dev, coords=coords, coords_out=eb.coords, gt=image, gt_out=eb.image,
                      batch_size=eb.bs, batch_counts=eb._counts_dev)
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            ms.append(e0.elapsed_time(e1))
    eb.epoch = None  # the buffers no longer hold an epoch of the fit
    by = kernel_bytes(eb.n)
    m = st.median(ms)
    return {"call_ms_median": m, "call_ms_min": min(ms), "call_ms_max": max(ms), "bytes": by,
            "useful_GBps": by["useful"] / m / 1e6, "worst_case_GBps": by["worst_case_line_amplified"] / m / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle_fit.json"))
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--time-rounds", type=int, default=6)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    image, coords, shape = make_kspace(*bench.SHAPE, seed=1234, normalization="coil")
    cfg = dict(bench.CONFIG)
    res = {"box": {"host": socket.gethostname(), "gpu": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "hip": torch.version.hip},
           "workload": {"config": cfg, "shape": list(bench.SHAPE), "rows": int(coords.shape[0]), "precision": "f32"}}
    print(f"data ready on {res['box']['host']}", flush=True)
    res["timing"], tr = step_times(cfg, image, coords, shape, dev, args.time_rounds)
    print(json.dumps(res["timing"]["median_step_ms"]), flush=True)
    res["inr_shuffle_epoch"] = kernel_time(tr, dev)
    print(json.dumps(res["inr_shuffle_epoch"]), flush=True)
    del tr
    res["psnr"] = psnr_runs(cfg, image, coords, shape, dev, args.epochs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("box", "timing", "inr_shuffle_epoch")}))
    print(json.dumps({k: v for k, v in res["psnr"].items() if k.startswith("shuffled_minus")}))


if __name__ == "__main__":
    main()
