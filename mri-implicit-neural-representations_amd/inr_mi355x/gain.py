"""Learned radial gain: the one operation that joins a backbone and a gain network the way the
reference's ``ScalerWrapper`` does (models/networks.py:380-405),

    res = backbone(gamma(coords)) * exp(-scaler(z)),        z = (coil coordinate, k-space radius)

with the loss on ``res`` and its gradients to both networks' outputs in one pass (csrc/inr_gain.hip).  Here: the input
of the gain network, the float64 statement of what the kernel computes (the oracle of tests/test_gpu_gain.py), and the
ctypes bindings on device tensors.  inr_mi355x/train_scaling.py drives the two engines; inr_mi355x/reconstruct.py
renders their checkpoints.

Per row, y = (y0, y1) the backbone's output, s the gain network's, t the target:
    g = exp(-s)      res_c = y_c g      (L, dres) = the pointwise loss of inr_loss_grad on (res, t)
    dy_c = dres_c g  ds = -(dres_0 res_0 + dres_1 res_1)
Rows with mask == 0 add nothing and get dy = ds = 0; res is made for every row.  The denominators |res| + eps of the
LogSpace / HDR / Center losses are detached, as in the reference (metrics/losses.py): dres is the gradient autograd gives.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import LossSpec, _ptr, _same_device, _shape


def gain_inputs(coords: torch.Tensor) -> torch.Tensor:
    """z [B,2] = (coords[:,0], sqrt(coords[:,1]^2 + coords[:,2]^2)): the coil coordinate and the k-space radius -- the
    two-column companion the reference's dataset offers (``coords[idx, [0, -1]]`` with cat_dists, data/nerp_datasets.py:
    387,392).  In torch on the data's device; the radius is formed as the trainers form ``dist``."""
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise RuntimeError(f"coords has shape {tuple(coords.shape)}, expected [B,3]")
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    return torch.stack((coords[:, 0], dist), dim=1).contiguous()


# ---- the float64 statement ---------------------------------------------------------------------------------------------
def loss_rows_float64(loss: LossSpec, y: np.ndarray, t: np.ndarray, inv: float, hdr_A: float = 0.0):
    """(L [n], g [n,2]) in float64: value and gradient of the pointwise loss of one row each -- the table of
    tests/loss_cases.py (``row_terms``), written out in plain numpy.  tests/test_gain_host.py holds it to that table and,
    through the composite, to torch.autograd on the oracle's loss functions in float64."""
    y, t = np.asarray(y, dtype=np.float64), np.asarray(t, dtype=np.float64)
    e = y - t
    kind = loss.kind
    with np.errstate(all="ignore"):
        if kind == L.LOSS_L2_HALF:
            return (e * e).sum(1) * inv / 4.0, e * inv / 2.0
        if kind == L.LOSS_L1_HALF:
            return np.abs(e).sum(1) * inv / 4.0, np.sign(e) * inv / 4.0
        if kind == L.LOSS_TANH:
            ty = np.tanh(y)
            d = ty - np.tanh(t)
            return (d * d).sum(1) * inv / 2.0, d * (1.0 - ty * ty) * inv
        if kind == L.LOSS_MSLE_HALF:
            ay = y + 1.0 + 1e-9
            d = np.log(ay) - np.log(t + 1.0 + 1e-9)
            return (d * d).sum(1) * inv / 4.0, d / ay * inv / 2.0
        ya2 = (y * y).sum(1)
        den = np.sqrt(ya2) + loss.eps
        ea2 = (e * e).sum(1)
        if kind == L.LOSS_LOGSPACE:
            q = inv / (den * den)
            return ea2 * q, 2.0 * e * q[:, None]
        if kind == L.LOSS_CENTER:  # the pointwise part (0.1 rel + 0.9 (rel + reg))
            q = inv / (den * den)
            rq = 0.9 * loss.factor * hdr_A * q
            return ea2 * q + rq * ya2, 2.0 * e * q[:, None] + 2.0 * rq[:, None] * y
        if kind == L.LOSS_HDR:
            lg = np.log(np.sqrt(ea2) / den)
            rq = loss.factor * hdr_A / (den * den)
            return (lg * lg + rq * ya2) * inv, (2.0 * lg / ea2)[:, None] * e * inv + 2.0 * rq[:, None] * y * inv
    raise ValueError(f"loss kind {kind}")


def gain_loss_grad_numpy(loss: LossSpec, y, s, gt, mask, count: int, hdr_A: float = 0.0
                         ) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
    """(loss, res [B,2], dy [B,2], ds [B]) in float64 for y [B,2], s [B], gt [B,2], mask [B] or None: the module
    docstring's definition.  ``count`` = rows entering the mean (the sampled rows)."""
    y, gt = np.asarray(y, dtype=np.float64).reshape(-1, 2), np.asarray(gt, dtype=np.float64).reshape(-1, 2)
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    B = len(s)
    if len(y) != B or len(gt) != B:
        raise ValueError(f"y {y.shape}, s {s.shape}, gt {gt.shape}")
    keep = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    g = np.exp(-s)
    res = y * g[:, None]
    dy, ds = np.zeros((B, 2)), np.zeros(B)
    total = 0.0
    if keep.any():
        Lr, dres = loss_rows_float64(loss, res[keep], gt[keep], 1.0 / float(count), hdr_A)
        total = float(np.sum(Lr))
        dy[keep] = dres * g[keep, None]
        ds[keep] = -(dres * res[keep]).sum(1)
    return total, res, dy, ds


# ---- the kernels -------------------------------------------------------------------------------------------------------
def gain_loss_grad(loss: LossSpec, y: torch.Tensor, s: torch.Tensor, gt: torch.Tensor, count: int,
                   mask: Optional[torch.Tensor] = None, hdr_A: float = 0.0, want_res: bool = True,
                   loss_out: Optional[torch.Tensor] = None):
    """inr_gain_loss_grad on device tensors y [B,2], s [B], gt [B,2], mask [B] uint8 or None -> (loss scalar view of
    ``loss_out`` (LOSS_WORDS floats; made when not given), res [B,2] or None, dy [B,2], ds [B])."""
    B = int(y.shape[0])
    _shape(y, "y", B, 2)
    _shape(s, "s", B)
    _shape(gt, "gt", B, 2)
    _shape(mask, "mask", B)
    if loss_out is None:
        loss_out = torch.zeros(L.LOSS_WORDS, device=y.device)
    _shape(loss_out, "loss_out", L.LOSS_WORDS)
    ins = (_ptr(y, "y"), _ptr(s, "s"), _ptr(gt, "gt"), _ptr(mask, "mask", torch.uint8), _ptr(loss_out, "loss_out"))
    _same_device(y, s=s, gt=gt, mask=mask, loss_out=loss_out)
    dy, ds = torch.empty_like(y), torch.empty_like(s)
    res = torch.empty_like(y) if want_res else None
    ld = loss.desc(1.0 / float(count), hdr_A)
    L.launch("inr_gain_loss_grad", y.device, C.byref(ld), ins[0], ins[1], ins[2], ins[3], B, _ptr(res, "res"), ins[4],
             _ptr(dy, "dy"), _ptr(ds, "ds"))
    return loss_out[0], res, dy, ds


def gain_apply(y: torch.Tensor, s: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_gain_apply: res [B,2] = y exp(-s) (no gradient); ``out`` may be ``y`` itself."""
    B = int(y.shape[0])
    _shape(y, "y", B, 2)
    _shape(s, "s", B)
    py, ps = _ptr(y, "y"), _ptr(s, "s")
    _same_device(y, s=s)
    res = torch.empty_like(y) if out is None else out
    _shape(res, "out", B, 2)
    _same_device(y, out=res)
    L.launch("inr_gain_apply", y.device, py, ps, B, _ptr(res, "out"))
    return res
