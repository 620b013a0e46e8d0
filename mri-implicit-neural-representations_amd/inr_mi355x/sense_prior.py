"""A total-variation prior on the IMAGE of a SENSE fit (no reference counterpart -- the
reference's tv_loss, ``inr_tv_grad`` / ``inr_loss_tv_grad`` here, is on a coil's predicted k-space and is no image prior).
In a SENSE fit the image I(y, x) exists on the device at every step, as the image network's output [H*W,2]; the prior is
smoothed isotropic TV of that complex image with forward differences that are zero past the last row / column:

    ax(p) = I[y][x+1] - I[y][x]      ay(p) = I[y+1][x] - I[y][x]
    n(p)  = sqrt(|ax|^2 + |ay|^2 + eps^2)
    TV    = (1 / (H W)) sum_p (n(p) - eps)
    u = ax / n,  v = ay / n           (both 0 where n = 0, which only eps = 0 can give)
    dTV/dI(p) = (1 / (H W)) (u(left of p) - u(p) + v(above p) - v(p))         (missing neighbours give 0)

Here: the fp32 numpy text of csrc/inr_image_tv.hip, operation for operation (``image_tv_numpy``: the gradient bit for
bit; the value is the fp64 sum of the same fp32 terms, scaled in fp64 and rounded once), the plain float64 statement
beside it (``image_tv_float64``), the ctypes binding on device tensors (``image_tv``) and the parser of
config['sense']['prior'] (``parse_prior``).  inr_mi355x/train_sense.py adds the prior to both SENSE step variants.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import _ptr, _same_device, _shape
from .sense import _f32

PRIOR_FIELDS = ("kind", "weight", "eps")
PRIOR_KINDS = ("tv",)
PRIOR_EPS = 1e-3  # in network units: the image network's last_tanh bounds |I| by 1.  A starting value, not tuned


# ---- settings ----------------------------------------------------------------------------------------------------------
def parse_prior(over) -> Optional[dict]:
    """config['sense']['prior'] -> None (absent, 'none', or kind: none) or {'kind': 'tv', 'weight': w > 0, 'eps': e >= 0}.
    ``kind`` defaults to 'tv' when a weight is given, ``eps`` to 1e-3.  ValueError for anything else: unknown keys, another
    kind, a missing, non-finite, zero or negative weight, a non-finite or negative eps."""
    where = "config['sense']['prior']"
    if over is None or (isinstance(over, str) and over.lower() == "none"):
        return None
    if not isinstance(over, dict):
        raise ValueError(f"{where} is a mapping of {list(PRIOR_FIELDS)} (or 'none'), got {over!r}")
    unknown = sorted(set(over) - set(PRIOR_FIELDS))
    if unknown:
        raise ValueError(f"{where} takes {list(PRIOR_FIELDS)}, got {unknown}")
    kind = over.get("kind", "tv" if "weight" in over else None)
    if kind is None or (isinstance(kind, str) and kind.lower() == "none"):
        if kind is None and over:
            raise ValueError(f"{where} = {over!r}: no 'kind' and no 'weight' (kind defaults to 'tv' when a weight is given)")
        return None
    if kind not in PRIOR_KINDS:
        raise ValueError(f"{where}['kind'] = {kind!r}: one of {list(PRIOR_KINDS)} (or 'none')")
    if "weight" not in over:
        raise ValueError(f"{where} has kind {kind!r} but no 'weight'")
    out = {"kind": kind}
    for key, default, positive in (("weight", None, True), ("eps", PRIOR_EPS, False)):
        raw = over.get(key, default)
        try:
            v = float(raw)
        except (TypeError, ValueError):
            raise ValueError(f"{where}[{key!r}] = {raw!r}: a number") from None
        if isinstance(raw, bool) or not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
            raise ValueError(f"{where}[{key!r}] = {raw!r}: finite and {'> 0' if positive else '>= 0'}")
        out[key] = v
    return out


def parse_prior_flag(arg: Optional[str]):
    """--sense-prior ARG -> what config['sense']['prior'] holds: 'none', or {'kind', 'weight'[, 'eps']} of
    KIND:WEIGHT[:EPS].  ValueError for another form; the numbers are checked by parse_prior."""
    if arg is None or arg.lower() == "none":
        return arg if arg is None else "none"
    parts = arg.split(":")
    if len(parts) not in (2, 3) or not all(parts):
        raise ValueError(f"--sense-prior {arg!r}: 'none' or KIND:WEIGHT[:EPS], for example tv:1e-3 or tv:1e-3:1e-4")
    try:
        numbers = [float(v) for v in parts[1:]]
    except ValueError:
        raise ValueError(f"--sense-prior {arg!r}: WEIGHT and EPS are numbers") from None
    over = dict(zip(("weight", "eps"), numbers), kind=parts[0])
    parse_prior(over)
    return over


# ---- the kernel in numpy -------------------------------------------------------------------------------------------------
def _scale(weight: float, H: int, W: int) -> np.float64:
    return np.float64(np.float32(weight)) / np.float64(H * W)


def _cells(img: np.ndarray, H: int, W: int, e2):
    """(n [H,W], ax, ay [H,W,2]) of the text: one fp32 operation per line"""
    ax, ay = np.zeros_like(img), np.zeros_like(img)
    ax[:, :-1] = img[:, 1:] - img[:, :-1]
    ay[:-1, :] = img[1:, :] - img[:-1, :]
    s0, s1 = ax[..., 0] * ax[..., 0], ax[..., 1] * ax[..., 1]
    s2, s3 = ay[..., 0] * ay[..., 0], ay[..., 1] * ay[..., 1]
    a, b = s0 + s1, s2 + s3
    q0 = a + b
    q = q0 + e2
    return np.sqrt(q), ax, ay


def image_tv_numpy(img, H: int, W: int, weight: float, eps: float, accumulate: bool = False,
                   dimg=None) -> Tuple[np.float32, np.ndarray]:
    """(value fp32, dimg [H*W,2] fp32): the text of inr_image_tv_grad.  The gradient is the kernel's, bit for bit (written,
    or added to ``dimg`` with one fp32 sum per component when ``accumulate``); the value is the fp64 sum of the kernel's
    fp32 terms n - eps times weight / (H W) in fp64, rounded once -- the kernel adds the same terms in another fixed
    order, so its value agrees to fp64 rounding."""
    img = _f32(img, H, W, 2)
    e, dt = np.float32(eps), img.dtype
    n, ax, ay = _cells(img, H, W, e * e)
    term = n - e
    value = np.float32(term.astype(np.float64).sum() * _scale(weight, H, W))
    c = np.float32(_scale(weight, H, W))
    ok = (n > 0)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ok, ax / n[..., None], dt.type(0))
        v = np.where(ok, ay / n[..., None], dt.type(0))
    ul, vu = np.zeros_like(u), np.zeros_like(v)
    ul[:, 1:] = u[:, :-1]
    vu[1:, :] = v[:-1, :]
    t0, t1 = ul - u, vu - v
    t = t0 + t1
    d = (c * t).reshape(H * W, 2)
    if accumulate:
        if dimg is None:
            raise ValueError("accumulate needs dimg")
        d = _f32(dimg, H * W, 2) + d
    return value, np.ascontiguousarray(d, dtype=np.float32)


def image_tv_terms(img, H: int, W: int, eps: float) -> np.ndarray:
    """fp32 [H,W]: the kernel's per-pixel terms n - eps"""
    e = np.float32(eps)
    return _cells(_f32(img, H, W, 2), H, W, e * e)[0] - e


def image_tv_float64(img, H: int, W: int, weight: float, eps: float) -> Tuple[float, np.ndarray]:
    """(weight * TV, weight * dTV/dimg [H*W,2]) in float64: the module docstring's formulas as they stand"""
    I = np.asarray(img, dtype=np.float64).reshape(H, W, 2)
    I = I[..., 0] + 1j * I[..., 1]
    ax, ay = np.zeros_like(I), np.zeros_like(I)
    ax[:, :-1] = I[:, 1:] - I[:, :-1]
    ay[:-1, :] = I[1:, :] - I[:-1, :]
    n = np.sqrt(np.abs(ax) ** 2 + np.abs(ay) ** 2 + float(eps) ** 2)
    safe = np.where(n > 0, n, 1.0)
    u, v = np.where(n > 0, ax / safe, 0.0), np.where(n > 0, ay / safe, 0.0)
    g = -(u + v)
    g[:, 1:] += u[:, :-1]
    g[1:, :] += v[:-1, :]
    k = float(weight) / (H * W)
    return k * float((n - float(eps)).sum()), k * np.stack((g.real, g.imag), axis=-1).reshape(H * W, 2)


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def image_tv(img: torch.Tensor, H: int, W: int, weight: float, eps: float, dimg: Optional[torch.Tensor] = None,
             accumulate: bool = False, loss_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_image_tv_grad on a device tensor img [H*W,2]: weight * dTV/dimg written (or, with ``accumulate``, added) into
    ``dimg`` [H*W,2] when given, and weight * TV returned as a 0-d view of ``loss_out`` ([LOSS_WORDS] floats, made when
    not given; the words after the first are the kernel's scratch)."""
    _shape(img, "img", H * W, 2)
    _shape(dimg, "dimg", H * W, 2)
    _shape(loss_out, "loss_out", L.LOSS_WORDS)
    if accumulate and dimg is None:
        raise RuntimeError("accumulate needs dimg")
    pi, pd = _ptr(img, "img"), _ptr(dimg, "dimg")  # host tensors: no CPU fallback
    loss_out = torch.empty(L.LOSS_WORDS, device=img.device) if loss_out is None else loss_out
    pl = _ptr(loss_out, "loss_out")
    _same_device(img, loss_out=loss_out, dimg=dimg)
    L.launch("inr_image_tv_grad", img.device, pi, H, W, float(weight), float(eps), int(bool(accumulate)), pl, pd)
    return loss_out[0]
