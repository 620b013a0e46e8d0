#!/usr/bin/env python3
"""Generate tests/golden/focal.npz + focal_meta.json by IMPORTING the reference's own FocalFrequencyLoss from
/root/reference/src (build container only; the reference never travels), the way tools/make_golden.py imports its classes.

What is written is data only: the inputs (B = 37 rows at amplitude 0.3, a fixed mask) and, per case, the loss the class
returned and the gradient torch.autograd gave for it, in float64 and in fp32.  The class is applied to what train.py:176-180
would hand it: ``out`` and ``gt`` [B,2], or ``out[mask]`` and ``gt[mask]``.  Run:  python tools/make_golden_focal.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/src"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

sys.dont_write_bytecode = True  # the reference tree is read-only: importing it must not leave __pycache__ behind
sys.path.insert(0, REF)
_fm = types.ModuleType("fastmri")  # metrics/losses.py imports fastmri at module scope; only RadialL2Loss calls it
_fm.complex_abs = lambda x: (x ** 2).sum(-1).sqrt()
sys.modules["fastmri"] = _fm

from metrics.losses import FocalFrequencyLoss  # noqa: E402

torch.set_num_threads(1)

B = 37
CASES = {  # name: (constructor arguments, prediction equals target, masked)
    "defaults": (dict(), False, False),
    "alpha_0.5": (dict(alpha=0.5), False, False),
    "alpha_2": (dict(alpha=2.0), False, False),
    "no_log": (dict(log_matrix=False), False, False),
    "weight_0.3": (dict(loss_weight=0.3), False, False),
    "equal": (dict(), True, False),
    "masked": (dict(), False, True),
}


def run(kw, out, gt, sel, dtype):
    o = torch.from_numpy(out).to(dtype).requires_grad_(True)
    t = torch.from_numpy(gt).to(dtype)
    loss = FocalFrequencyLoss(**kw)(o[sel], t[sel]) if sel is not None else FocalFrequencyLoss(**kw)(o, t)
    (g,) = torch.autograd.grad(loss, o)
    return loss.detach().numpy().copy(), g.numpy().copy()


def main():
    rng = np.random.RandomState(20211012)
    out = (rng.uniform(-1.0, 1.0, (B, 2)) * 0.3).astype(np.float32)
    gt = (rng.uniform(-1.0, 1.0, (B, 2)) * 0.3).astype(np.float32)
    mask = (rng.uniform(size=B) > 0.4).astype(np.uint8)
    mask[int(np.argmax(((out - gt) ** 2).sum(1)))] = 0  # the row of largest error is NOT sampled
    arrays = dict(out=out, gt=gt, mask=mask)
    meta = dict(B=B, amplitude=0.3, cases={})
    for name, (kw, equal, masked) in CASES.items():
        o = gt.copy() if equal else out
        sel = torch.from_numpy(mask.astype(bool)) if masked else None
        l64, g64 = run(kw, o, gt, sel, torch.float64)
        l32, g32 = run(kw, o, gt, sel, torch.float32)
        arrays.update({f"{name}.loss64": l64, f"{name}.grad64": g64, f"{name}.loss32": l32, f"{name}.grad32": g32})
        full = dict(alpha=1.0, log_matrix=True, loss_weight=1.0)
        full.update(kw)
        meta["cases"][name] = dict(full, equal=equal, masked=masked, count=int(mask.sum()) if masked else B)
    np.savez(os.path.join(OUT, "focal.npz"), **arrays)
    with open(os.path.join(OUT, "focal_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote focal.npz:", sorted(arrays))


if __name__ == "__main__":
    main()
