#!/usr/bin/env python
"""Generate tests/golden/ring_norm.npz by RUNNING the reference's own scale_space
(train_variations/train_normalize_per_bucket.py:20-27) forward and inverse on a few small cases (build container only:
needs the reference checkout).

    python tools/make_golden_ring_norm.py /path/to/reference/src      (or INR_REFERENCE_SRC=/path/to/reference/src)

The function is taken out of the reference file with ``ast`` at run time and executed (the file itself cannot be
imported: it parses a command line and trains at module level); nothing of its text is kept.  The fixture holds arrays
only.  Per case ``<tag>``: dist [n] fp32, values [n,2] fp32, radii [K+1] fp64, divisors [K] fp32, forward [n,2] fp32 =
scale_space(divisors, values, dist, radii), inverse [n,2] fp32 = scale_space([1 / d], forward, dist, radii) with the
reciprocals formed as the reference forms stats_rec (line 131: ``1 / x`` on 0-dim fp32 tensors).
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_scale_space(ref_src):
    path = os.path.join(ref_src, "train_variations", "train_normalize_per_bucket.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "scale_space"]
    if len(fn) != 1:
        sys.exit(f"{path}: expected one scale_space, found {len(fn)}")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["scale_space"]


def run(scale_space, dist, values, radii, divisors):
    """forward and inverse as the reference's script applies them (lines 125-131, 144, 213)"""
    d = torch.from_numpy(dist)
    stats = torch.from_numpy(divisors)  # partition_and_stats hands back fp32 tensors: stats[i] is a 0-dim tensor
    stats_rec = [1 / x for x in stats]
    fwd = scale_space(stats, torch.from_numpy(values.copy()), d, radii).numpy().copy()
    inv = scale_space(stats_rec, torch.from_numpy(fwd.copy()), d, radii).numpy().copy()
    return fwd, inv


def fl32_below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def cases():
    rng = np.random.default_rng(2024)
    normal = lambda n: (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-6, 2, (n, 1)))).astype(np.float32)
    # the probe: a 2 x 12 x 10 grid, four rings of which one is empty, plus rows exactly on a radius, one fp32 step below
    # one, beyond the last radius and NaN
    ys, xs = np.linspace(-1, 1, 12, dtype=np.float32), np.linspace(-1, 1, 10, dtype=np.float32)
    grid = np.sqrt((ys[:, None] ** 2 + xs[None, :] ** 2).astype(np.float32)).astype(np.float32)
    radii = np.array([0.0, 0.4, 0.4, 0.9, 1.3], dtype=np.float64)
    extra = np.array([0.0, 0.4, fl32_below(0.4), 0.9, fl32_below(0.9), 1.3, fl32_below(1.3), 1.4, 5.0, np.nan, -0.25],
                     dtype=np.float32)
    dist = np.concatenate([np.tile(grid.reshape(-1), 2), extra]).astype(np.float32)
    yield "probe", dist, normal(dist.size), radii, np.array([3.7, 11.0, 0.62, 0.013], dtype=np.float32)
    # 64 rings of sqrt(2) / 64, the last one open to 5 as the partition leaves it
    radii = np.sqrt(2.0) * np.arange(65) / 64.0
    radii[64] = 5.0
    dist = np.concatenate([rng.uniform(0, 1.5, 60), radii[:-1], [fl32_below(r) for r in radii[1:]]]).astype(np.float32)
    yield "rings64", dist, normal(dist.size), radii, np.exp(rng.uniform(-7, 1, 64)).astype(np.float32)
    # one ring that leaves rows outside on both sides
    dist = np.concatenate([rng.uniform(0, 1.5, 61), [0.25, 1.0, np.nan]]).astype(np.float32)
    yield "ring1", dist, normal(dist.size), np.array([0.25, 1.0]), np.array([0.37], dtype=np.float32)


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("INR_REFERENCE_SRC")
    if not ref_src:
        sys.exit("usage: make_golden_ring_norm.py REFERENCE_SRC")
    scale_space = reference_scale_space(ref_src)
    arrs = {}
    for tag, dist, values, radii, divisors in cases():
        fwd, inv = run(scale_space, dist, values, radii, divisors)
        for k, v in dict(dist=dist, values=values, radii=radii, divisors=divisors, forward=fwd, inverse=inv).items():
            arrs[f"{tag}/{k}"] = v
    out = os.path.join(ROOT, "tests", "golden", "ring_norm.npz")
    np.savez_compressed(out, **arrs)
    print(out, os.path.getsize(out), "bytes;", ", ".join(f"{t}: {arrs[t + '/dist'].size} rows" for t in ("probe", "rings64", "ring1")))


if __name__ == "__main__":
    main()
