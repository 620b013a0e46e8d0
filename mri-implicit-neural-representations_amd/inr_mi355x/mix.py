"""Mixture of heads: the one operation that joins K expert networks and a gate network the way
the reference's ``MultiHeadWrapper`` does with ``backbone=None`` (models/networks.py:275-328),

    res = clamp(sum_k w_k y_k, -1, 1),      y_k = expert_k(gamma(coords)),  w = gate(z),  z = (coil coordinate, radius)

with the loss of one batch (train_multihead_fast.py:178-203, cleaned up: INTEGRATION.md section 4)

    total = L(res, gt; live rows, mean over count_0) + sum_k L(y_k, gt; live rows of ring k, mean over count_k)

and its gradients to every network's output in one pass (csrc/inr_mix.hip).  Here: the float64 statement of what the
kernel computes (the oracle of tests/test_gpu_mix.py), the float32 statement of ``res`` (which the kernel equals bit for
bit), the per-ring row counts, and the ctypes bindings on device tensors.  inr_mi355x/train_multihead.py drives the
K + 1 engines; inr_mi355x/reconstruct.py renders their checkpoints.

Per row, y_k = (y_k0, y_k1) expert k's output, w_k the gate's, d the k-space radius, t the target:
    pre_c = sum_k w_k y_kc (head order)    res_c = clamp ? min(max(pre_c, -1), 1) : pre_c
    (L_0, dres) = the pointwise loss of inr_loss_grad on (res, t), mean over count_0
    dpre_c = dres_c where not clamp or -1 <= pre_c <= 1 (both ends included, as torch.clamp), else 0
    dw_k = dpre_0 y_k0 + dpre_1 y_k1
    ring k (radii[k] <= d <= radii[k+1], both ends included: an edge row is in two rings):
        (L_{1+k}, g_k) = the same pointwise loss on (y_k, t), mean over count_k;  g_k = 0 off the ring
    dy_k = g_k                       (detach: the mixed term reaches the gate alone, the wrapper's detach_outs=True)
    dy_k = g_k + w_k dpre            (joint training)
Rows with mask == 0 add nothing and get dy = dw = 0; res is made for every row.  A ring without a live row adds nothing.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import LossSpec, _ptr, _same_device, _shape
from .gain import loss_rows_float64

MAX_HEADS = L.MIX_MAX_HEADS


def _check_heads(K: int) -> int:
    K = int(K)
    if K < 2 or K > MAX_HEADS:
        raise ValueError(f"a mixture has 2..{MAX_HEADS} heads, got {K}")
    return K


def check_radii(radii: Sequence[float], K: int) -> List[float]:
    """the K + 1 ring edges as floats; they must increase"""
    radii = [float(r) for r in radii]
    if len(radii) != K + 1:
        raise ValueError(f"{K} heads need {K + 1} radii, got {len(radii)}")
    if any(not (b > a) for a, b in zip(radii, radii[1:])):
        raise ValueError(f"radii must increase, got {radii}")
    return radii


def ring_membership(dist: np.ndarray, radii: Sequence[float]) -> np.ndarray:
    """bool [K, B]: row b lies in ring k, radii[k] <= dist[b] <= radii[k+1] compared in float32 as the kernel compares"""
    d = np.asarray(dist, dtype=np.float32).reshape(-1)
    r = np.asarray(radii, dtype=np.float32)
    return np.stack([(d >= r[k]) & (d <= r[k + 1]) for k in range(len(r) - 1)])


def ring_counts(dist, mask, radii: Sequence[float], lo: int = 0, hi: Optional[int] = None) -> List[int]:
    """[count_0, count_1 .. count_K] of the rows [lo, hi): the live rows (mask != 0; all of them without a mask), then
    the live rows of each ring.  ``dist`` / ``mask``: numpy arrays or torch tensors on any device."""
    if isinstance(dist, torch.Tensor):
        dist = dist.detach().cpu().numpy()
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    d = np.asarray(dist).reshape(-1)[lo:hi]
    live = np.ones(len(d), dtype=bool) if mask is None else np.asarray(mask).reshape(-1)[lo:hi] != 0
    rings = ring_membership(d, radii)
    return [int(live.sum())] + [int((live & m).sum()) for m in rings]


def inv_counts(counts: Sequence[int]) -> List[float]:
    """1 / count per term; 0 where nothing is counted (the term then has no row)"""
    return [1.0 / float(c) if c > 0 else 0.0 for c in counts]


# ---- the float32 and float64 statements --------------------------------------------------------------------------------
def mix_numpy_f32(ys: Sequence[np.ndarray], w: np.ndarray, clamp: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """(pre [B,2], res [B,2]) with every operation rounded in float32: the products w_k y_k, their sum in head order,
    the clamp.  inr_mix_loss_grad's and inr_mix_apply's res equal ``res`` bit for bit."""
    w = np.asarray(w, dtype=np.float32)
    K = _check_heads(len(ys))
    ys = [np.asarray(y, dtype=np.float32).reshape(-1, 2) for y in ys]
    w = w.reshape(len(ys[0]), K)
    pre = (w[:, 0:1] * ys[0]).astype(np.float32)
    for k in range(1, K):
        pre = (pre + (w[:, k:k + 1] * ys[k]).astype(np.float32)).astype(np.float32)
    res = np.minimum(np.maximum(pre, np.float32(-1.0)), np.float32(1.0)) if clamp else pre.copy()
    return pre, res.astype(np.float32)


def mix_loss_grad_numpy(loss: LossSpec, ys: Sequence[np.ndarray], w, gt, dist, mask, radii: Sequence[float],
                        counts: Optional[Sequence[int]] = None, detach: bool = True, clamp: bool = True,
                        hdr_A: float = 0.0):
    """(total, terms [K+1], pre [B,2], res [B,2], dys K x [B,2], dw [B,K]) in float64: the module docstring's definition.
    ``counts`` = [count_0 .. count_K] (default: ring_counts of these rows)."""
    K = _check_heads(len(ys))
    radii = check_radii(radii, K)
    ys = [np.asarray(y, dtype=np.float64).reshape(-1, 2) for y in ys]
    B = len(ys[0])
    w = np.asarray(w, dtype=np.float64).reshape(B, K)
    gt = np.asarray(gt, dtype=np.float64).reshape(B, 2)
    live = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    rings = ring_membership(dist, radii)
    if counts is None:
        counts = ring_counts(dist, mask, radii)
    inv = inv_counts(counts)
    pre = np.zeros((B, 2))
    for k in range(K):
        pre = pre + w[:, k:k + 1] * ys[k]
    res = np.clip(pre, -1.0, 1.0) if clamp else pre.copy()
    dys, dw = [np.zeros((B, 2)) for _ in range(K)], np.zeros((B, K))
    terms = [0.0] * (K + 1)
    if live.any():
        Lr, dres = loss_rows_float64(loss, res[live], gt[live], inv[0], hdr_A)
        terms[0] = float(np.sum(Lr))
        dpre = np.zeros((B, 2))
        dpre[live] = dres
        if clamp:
            dpre = np.where((pre >= -1.0) & (pre <= 1.0), dpre, 0.0)
        for k in range(K):
            dw[:, k] = (dpre * ys[k]).sum(1)
            if not detach:
                dys[k] += w[:, k:k + 1] * dpre
    for k in range(K):
        sel = live & rings[k]
        if sel.any():
            Lr, g = loss_rows_float64(loss, ys[k][sel], gt[sel], inv[1 + k], hdr_A)
            terms[1 + k] = float(np.sum(Lr))
            dys[k][sel] += g
    return float(sum(terms)), terms, pre, res, dys, dw


# ---- the kernels -------------------------------------------------------------------------------------------------------
def _desc(ys: Sequence[torch.Tensor], dys: Optional[Sequence[torch.Tensor]], radii: Optional[Sequence[float]],
          inv: Optional[Sequence[float]], detach: bool, clamp: bool) -> L.MixDesc:
    K = _check_heads(len(ys))
    B = int(ys[0].shape[0])
    d = L.MixDesc(n_heads=K, detach=int(bool(detach)), clamp=int(bool(clamp)))
    for k, y in enumerate(ys):
        _shape(y, f"y[{k}]", B, 2)
        d.y[k] = _ptr(y, f"y[{k}]")
        _same_device(ys[0], **{f"y[{k}]": y})
        if dys is not None:
            d.dy[k] = _ptr(dys[k], f"dy[{k}]")
    if radii is not None:
        for k, r in enumerate(check_radii(radii, K)):
            d.radii[k] = r
        if len(inv) != K + 1:
            raise ValueError(f"{K} heads need {K + 1} inv_counts, got {len(inv)}")
        for k, v in enumerate(inv):
            d.inv_count[k] = float(v)
    return d


def mix_loss_grad(loss: LossSpec, ys: Sequence[torch.Tensor], w: torch.Tensor, gt: torch.Tensor, dist: torch.Tensor,
                  radii: Sequence[float], inv_count: Sequence[float], mask: Optional[torch.Tensor] = None,
                  detach: bool = True, clamp: bool = True, hdr_A: float = 0.0, want_res: bool = True,
                  loss_out: Optional[torch.Tensor] = None):
    """inr_mix_loss_grad on device tensors ys K x [B,2], w [B,K], gt [B,2], dist [B], mask [B] uint8 or None;
    ``inv_count`` = [1/count_0 .. 1/count_K] (0: no row) -> (loss_out (LOSS_WORDS floats, made when not given: word 0 the
    total, words 1 .. K+1 the terms), res [B,2] or None, dys K x [B,2], dw [B,K])."""
    K = _check_heads(len(ys))
    B = int(ys[0].shape[0])
    dev = ys[0].device
    _shape(w, "w", B, K)
    _shape(gt, "gt", B, 2)
    _shape(dist, "dist", B)
    _shape(mask, "mask", B)
    if loss_out is None:
        loss_out = torch.zeros(L.LOSS_WORDS, device=dev)
    _shape(loss_out, "loss_out", L.LOSS_WORDS)
    _same_device(ys[0], w=w, gt=gt, dist=dist, mask=mask, loss_out=loss_out)
    dys = [torch.empty_like(y) for y in ys]
    dw = torch.empty_like(w)
    res = torch.empty_like(ys[0]) if want_res else None
    d = _desc(ys, dys, radii, inv_count, detach, clamp)
    ld = loss.desc(float(inv_count[0]), hdr_A)
    L.launch("inr_mix_loss_grad", dev, C.byref(ld), C.byref(d), _ptr(w, "w"), _ptr(gt, "gt"), _ptr(dist, "dist"),
             _ptr(mask, "mask", torch.uint8), B, _ptr(res, "res"), _ptr(loss_out, "loss_out"), _ptr(dw, "dw"))
    return loss_out, res, dys, dw


def mix_apply(ys: Sequence[torch.Tensor], w: torch.Tensor, clamp: bool = True,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_mix_apply: res [B,2] = clamp(sum_k w_k y_k) (no gradient); ``out`` may be ``ys[0]`` itself."""
    K = _check_heads(len(ys))
    B = int(ys[0].shape[0])
    _shape(w, "w", B, K)
    pw = _ptr(w, "w")
    res = torch.empty_like(ys[0]) if out is None else out
    _shape(res, "out", B, 2)
    _same_device(ys[0], w=w, out=res)
    d = _desc(ys, None, None, None, True, clamp)
    L.launch("inr_mix_apply", w.device, C.byref(d), pw, B, _ptr(res, "out"))
    return res
