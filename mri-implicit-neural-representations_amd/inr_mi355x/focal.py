"""Focal frequency loss (``loss: FFL``): the reference's ``FocalFrequencyLoss`` (metrics/losses.py:
57-119; Jiang et al., ICCV 2021) with the online weight matrix, applied to what train.py:176-180 would hand it -- the
network's k-space rows ``out`` and the targets ``gt`` [B,2], the sampled rows where there is a mask.  The model predicts
k-space rows, so the "frequency distance" is the row's squared error, and every row is weighted by its own error relative
to the largest of the batch:

    e_o = out_o - gt_o      q = e_0^2 + e_1^2
    m   = sqrt(q)^alpha     n = log(m + 1) if log_matrix else m          n_max = max over the sampled rows of n
    w   = 0 if n_max == 0 else clamp(n / n_max, 0, 1)                     DETACHED: a constant of the step
    loss   = loss_weight / N * sum_r w_r q_r                              N = sampled rows
    dout_o = loss_weight * 2 * w * e_o / N                                unsampled rows: 0, not in n_max, not in the sum

n_max == 0 is the reference's ``matrix_tmp[isnan] = 0`` (0 / 0 when prediction equals target everywhere): loss and gradient
are 0.  ``batch_matrix`` changes nothing in the reference (both branches are the same line) and has no key here; a
caller-supplied matrix is not supported.  Here: the config keys, the ctypes binding of inr_focal_loss_grad
(csrc/inr_loss_focal.hip) on device tensors -- there is no CPU path -- and the statement of the kernel in numpy, in float64
and operation by operation in fp32 (the oracle of tests/test_gpu_focal.py).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import _ptr, _same_device, _shape

KEYS = ("ffl_alpha", "ffl_log_matrix", "ffl_weight")


@dataclass(frozen=True)
class FocalSpec:
    """The reference constructor's arguments and defaults (metrics/losses.py:72)."""
    alpha: float = 1.0
    log_matrix: bool = True
    loss_weight: float = 1.0

    def __post_init__(self):
        if not (math.isfinite(self.alpha) and self.alpha > 0.0):
            raise ValueError(f"ffl_alpha = {self.alpha!r} (must be finite and > 0)")
        if not math.isfinite(self.loss_weight):
            raise ValueError(f"ffl_weight = {self.loss_weight!r} (must be finite)")

    @staticmethod
    def from_opts(opts: Optional[dict]) -> "FocalSpec":
        """config['loss_opts']: ffl_alpha (1.0), ffl_log_matrix (true), ffl_weight (1.0); any other ffl_* key is a
        ValueError (a misspelt key would otherwise leave its default in force without a word)."""
        opts = opts or {}
        unknown = sorted(k for k in opts if str(k).startswith("ffl_") and k not in KEYS)
        if unknown:
            raise ValueError(f"loss_opts: unknown key(s) {unknown} (the focal frequency loss takes {list(KEYS)})")
        lm = opts.get("ffl_log_matrix", True)
        if not isinstance(lm, (bool, np.bool_)):
            raise ValueError(f"ffl_log_matrix = {lm!r} (true or false)")
        return FocalSpec(float(opts.get("ffl_alpha", 1.0)), bool(lm), float(opts.get("ffl_weight", 1.0)))

    def summary(self) -> dict:
        return {"alpha": self.alpha, "log_matrix": self.log_matrix, "loss_weight": self.loss_weight}


# ---- the statement in numpy --------------------------------------------------------------------------------------------
def _fold32(terms: np.ndarray, live: np.ndarray) -> np.float32:
    """the kernel's sum of the per-row terms in fp32: FOCAL_BLOCKS contiguous ranges of row pairs, lane j of a block adds
    the rows of its pairs lo + j, lo + j + 256, ... in order (first row, then second; unsampled rows are skipped), the
    256-lane tree, then the partials in block order"""
    f = np.float32
    B = len(terms)
    pairs = (B + 1) // 2
    per = -(-pairs // L.FOCAL_BLOCKS)
    t = np.zeros(2 * pairs, dtype=f)
    t[:B] = np.where(live, terms, f(0))
    total = f(0)
    with np.errstate(all="ignore"):
        for b in range(L.FOCAL_BLOCKS):
            lo, hi = min(b * per, pairs), min(b * per + per, pairs)
            lanes = np.zeros(256, dtype=f)
            for p0 in range(lo, hi, 256):
                k = min(256, hi - p0)
                rows = t[2 * p0:2 * (p0 + k)].reshape(k, 2)
                lanes[:k] = lanes[:k] + rows[:, 0]
                lanes[:k] = lanes[:k] + rows[:, 1]
            s = 128
            while s > 0:
                lanes[:s] = lanes[:s] + lanes[s:2 * s]
                s //= 2
            total = f(total + lanes[0])
    return total


def focal_loss_numpy(spec: FocalSpec, out, gt, count: int, mask=None, dtype=np.float64
                     ) -> Tuple[float, np.ndarray, float]:
    """(loss, dout [B,2], n_max) of the module docstring's definition.  ``dtype=np.float64``: the float64 statement (sums by
    numpy).  ``dtype=np.float32``: the kernel operation by operation -- every product, sum, quotient and square root
    rounded to fp32 in the kernel's order, pow and log taken in float64 and rounded once, the loss summed in the kernel's
    fixed scheme, inv = fp32(1 / count)."""
    f = np.dtype(dtype).type
    if f not in (np.float64, np.float32):
        raise ValueError(f"dtype {dtype!r}: float64 or float32")
    out, gt = np.asarray(out, dtype=f).reshape(-1, 2), np.asarray(gt, dtype=f).reshape(-1, 2)
    B = len(out)
    if len(gt) != B:
        raise ValueError(f"out {out.shape}, gt {gt.shape}")
    live = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if len(live) != B:
        raise ValueError(f"mask has {len(live)} entries, out {B} rows")
    alpha, lw, inv = f(spec.alpha), f(spec.loss_weight), f(1.0 / float(count))
    with np.errstate(all="ignore"):
        e = out - gt
        q = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        m = np.sqrt(q)
        if spec.alpha != 1.0:
            m = np.power(m.astype(np.float64), np.float64(alpha)).astype(f)
        if spec.log_matrix:
            n = np.log((m + f(1)).astype(np.float64)).astype(f)  # the sum m + 1 is rounded in the working precision
        else:
            n = m
        n_max = f(n[live].max()) if live.any() else f(0)
        if n_max == 0:
            w = np.zeros(B, dtype=f)
        else:
            w = np.minimum(np.maximum(n / n_max, f(0)), f(1))
        w = np.where(live, w, f(0))
        terms = w * q
        if f is np.float32:
            loss = f(f(_fold32(terms, live) * inv) * lw)
        else:
            loss = float(np.sum(terms[live])) * inv * lw
        dout = (((lw * f(2)) * e) * w[:, None]) * inv
        dout = np.where(live[:, None], dout, f(0))
    return (loss if f is np.float32 else float(loss)), dout, (n_max if f is np.float32 else float(n_max))


# ---- the kernel --------------------------------------------------------------------------------------------------------
def focal_loss_grad(spec: FocalSpec, out: torch.Tensor, gt: torch.Tensor, count: int,
                    mask: Optional[torch.Tensor] = None, want_grad: bool = True,
                    loss_out: Optional[torch.Tensor] = None):
    """inr_focal_loss_grad on device tensors out, gt [B,2] (fp32), mask [B] uint8 or None -> (loss: a scalar view of
    ``loss_out`` (LOSS_WORDS floats; made when not given), dout [B,2] or None when ``want_grad`` is false).  ``count`` = the
    sampled rows (the N of the mean).  Three launches on the current stream, no sync."""
    if out.dim() != 2:
        raise RuntimeError(f"out has shape {tuple(out.shape)}, expected [B,2]")
    B = int(out.shape[0])
    _shape(out, "out", B, 2)
    _shape(gt, "gt", B, 2)
    _shape(mask, "mask", B)
    if B < 1 or int(count) < 1:
        raise RuntimeError(f"B = {B}, count = {count} (both must be >= 1)")
    p_out, p_gt, p_mask = _ptr(out, "out"), _ptr(gt, "gt"), _ptr(mask, "mask", torch.uint8)
    if loss_out is None:
        loss_out = torch.zeros(L.LOSS_WORDS, device=out.device)
    _shape(loss_out, "loss_out", L.LOSS_WORDS)
    p_loss = _ptr(loss_out, "loss_out")
    _same_device(out, gt=gt, mask=mask, loss_out=loss_out)
    dout = torch.empty_like(out) if want_grad else None
    d = L.FocalDesc(alpha=spec.alpha, log_matrix=int(spec.log_matrix), loss_weight=spec.loss_weight,
                    inv_count=1.0 / float(count))
    L.launch("inr_focal_loss_grad", out.device, C.byref(d), p_out, p_gt, p_mask, B, p_loss, _ptr(dout, "dout"))
    return loss_out[0], dout
