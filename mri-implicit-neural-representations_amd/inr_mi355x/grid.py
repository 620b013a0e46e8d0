"""Coordinate grids made on the device, a chunk of rows at a time (inr_grid_rows, csrc/inr_grid.hip):
what create_coords (data/utils.py:98-108) materialises whole on the host at 12 B per row and uploads.

Row ``r = (k*H + y)*W + x`` of the flattened (k, y, x) grid is
``(v(coils[k]; -1, 1, coils_total), v(y; y0, y1, H), v(x; x0, x1, W))`` and ``dist = sqrt(y*y + x*x)`` of the values, with

    v(i; a, b, n) = a                        when n == 1,
                    a + step*i               for i < n // 2,
                    b - step*(n - 1 - i)     for the rest,        step = (b - a) / (n - 1),

in fp32, every operation rounded on its own.  This is the grid's own definition, pinned by ``grid_rows_numpy`` the way
shuffle.epoch_order pins the permutation: torch.linspace on the CPU is not a fixed function of its arguments (its
vectorised path picks the half-formula per SIMD vector, so values depend on the host's vector width), and differs from
this formula by at most 2^-24 on [-1, 1].

What the grid means depends on the domain of the fit.  In image-space configs (config['transform']) a finer grid is
super-resolution and a window is a zoom.  In k-space configs a finer grid over the same window samples k-space more
densely -- a larger field of view after the inverse FFT -- and a narrower window keeps the low frequencies only -- a
lower-resolution image.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

MAX_COILS = 64  # coils per inr_grid_rows call (inr_grid_desc.coils)
MAX_CALL_ROWS = (1 << 31) - 1  # rows per inr_grid_rows call


class GridSpec:
    """Which grid: ``coils_total`` = C of the fit (the coil axis is v(c; -1, 1, C)), ``H`` x ``W`` points per coil over
    ``window`` = (y0, y1, x0, x1) (the fit's own grid: -1, 1, -1, 1), ``coils`` = which coils, in output order (default:
    all of them).  Values are checked where they are used (the library refuses a bad description with its own message)."""

    def __init__(self, coils_total: int, H: int, W: int, coils: Optional[Sequence[int]] = None,
                 window: Sequence[float] = (-1.0, 1.0, -1.0, 1.0)):
        self.coils_total, self.H, self.W = int(coils_total), int(H), int(W)
        self.coils = list(range(self.coils_total)) if coils is None else [int(c) for c in coils]
        if len(window) != 4:
            raise ValueError(f"window is (y0, y1, x0, x1), got {tuple(window)!r}")
        self.window = tuple(float(v) for v in window)

    @property
    def shape(self) -> Tuple[int, int, int]:
        return len(self.coils), self.H, self.W

    @property
    def rows(self) -> int:
        return len(self.coils) * self.H * self.W

    def __repr__(self) -> str:
        return f"GridSpec(coils_total={self.coils_total}, H={self.H}, W={self.W}, coils={self.coils}, window={self.window})"


def resolve_size(H: int, W: int, height: Optional[int] = None, width: Optional[int] = None,
                 scale: Optional[float] = None) -> Tuple[int, int]:
    """Points per axis of a rendered grid: ``scale`` multiplies H and W (rounded to the nearest integer, never below
    1); ``height`` / ``width`` override it."""
    h, w = int(H), int(W)
    if scale is not None:
        if not (float(scale) > 0.0) or not math.isfinite(float(scale)):
            raise ValueError(f"scale must be a positive number, got {scale!r}")
        h = max(1, int(math.floor(H * float(scale) + 0.5)))
        w = max(1, int(math.floor(W * float(scale) + 0.5)))
    if height is not None:
        h = int(height)
    if width is not None:
        w = int(width)
    if h < 1 or w < 1:
        raise ValueError(f"a grid needs at least one point per axis, got {h} x {w}")
    return h, w


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def axis_values_numpy(idx, a: float, b: float, n: int) -> np.ndarray:
    """v(i; a, b, n) for the integer indices ``idx``: float32 arithmetic, no float64 intermediate."""
    idx = np.asarray(idx, dtype=np.int64)
    a32, b32 = np.float32(a), np.float32(b)
    if n == 1:
        return np.full(idx.shape, a32, dtype=np.float32)
    step = np.float32(np.float32(b32 - a32) / np.float32(n - 1))
    lower = (a32 + (step * idx.astype(np.float32)).astype(np.float32)).astype(np.float32)
    upper = (b32 - (step * (n - 1 - idx).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.where(idx < n // 2, lower, upper).astype(np.float32)


def _check_spec(spec: GridSpec) -> None:
    if spec.H < 1 or spec.W < 1 or len(spec.coils) < 1 or spec.coils_total < 1:
        raise ValueError(f"{spec!r}: H, W, the number of coils and coils_total must be >= 1")
    if any(c < 0 or c >= spec.coils_total for c in spec.coils):
        raise ValueError(f"{spec!r}: a coil index is outside [0, {spec.coils_total})")
    if not all(math.isfinite(v) for v in spec.window):
        raise ValueError(f"{spec!r}: non-finite window")


def grid_rows_numpy(spec: GridSpec, lo: int, hi: int):
    """(coords [hi-lo,3], dist [hi-lo]) float32: rows [lo, hi) of the grid, by the definition above."""
    _check_spec(spec)
    if not 0 <= lo <= hi <= spec.rows:
        raise ValueError(f"rows [{lo}, {hi}) of a grid of {spec.rows}")
    y0, y1, x0, x1 = spec.window
    r = np.arange(lo, hi, dtype=np.int64)
    x = r % spec.W
    y = (r // spec.W) % spec.H
    k = r // (spec.W * spec.H)
    coil = np.asarray(spec.coils, dtype=np.int64)[k] if hi > lo else k
    vy = axis_values_numpy(y, y0, y1, spec.H)
    vx = axis_values_numpy(x, x0, x1, spec.W)
    coords = np.stack((axis_values_numpy(coil, -1.0, 1.0, spec.coils_total), vy, vx), axis=1).astype(np.float32)
    dist = np.sqrt(((vy * vy).astype(np.float32) + (vx * vx).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return coords, dist


# ---- the kernel --------------------------------------------------------------------------------------------------------
def _desc(spec: GridSpec) -> L.GridDesc:
    d = L.GridDesc()
    d.coils_total, d.n_coils, d.H, d.W = spec.coils_total, len(spec.coils), spec.H, spec.W
    for k, c in enumerate(spec.coils[:MAX_COILS]):  # (more than 64: the library refuses n_coils)
        d.coils[k] = c
    d.y0, d.y1, d.x0, d.x1 = spec.window
    return d


def _buffer(t: Optional[torch.Tensor], name: str, shape, device) -> torch.Tensor:
    if t is None:
        return torch.empty(*shape, device=device, dtype=torch.float32)
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the grid kernel only runs on an MI355X (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def grid_rows(spec: GridSpec, lo: int, hi: int, coords_out: Optional[torch.Tensor] = None,
              dist_out: Optional[torch.Tensor] = None, with_dist: bool = True, device="cuda"):
    """Rows [lo, hi) of the grid by inr_grid_rows on the current stream -> (coords [hi-lo,3], dist [hi-lo]) fp32 device
    tensors (``with_dist=False``: dist is not made, None comes back).  Buffers given by the caller are used as they are:
    nothing is allocated then, nothing is read back, one launch (graph-capturable).  hi - lo < 2^31 per call."""
    lo, hi = int(lo), int(hi)
    n = hi - lo
    if coords_out is not None:
        device = coords_out.device
    elif dist_out is not None:
        device = dist_out.device
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"grid_rows on {device}: the grid kernel only runs on an MI355X (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if dist_out is not None and not with_dist:
        raise RuntimeError("dist_out given with with_dist=False")
    rows = max(n, 0)
    coords_out = _buffer(coords_out, "coords_out", (rows, 3), device)
    dist = _buffer(dist_out, "dist_out", (rows,), device) if with_dist else None
    if dist is not None and dist.device != coords_out.device:
        raise RuntimeError(f"dist_out is on {dist.device}, coords_out on {coords_out.device}")
    d = _desc(spec)
    # (an empty tensor's data_ptr is 0: hand the library a real address so that a bad description is still refused)
    cp = coords_out.data_ptr() or None
    if cp is None and rows == 0:
        cp = torch.empty(4, device=device).data_ptr()
    L.launch("inr_grid_rows", device, d, lo, n, cp, None if dist is None else (dist.data_ptr() or None))
    return coords_out, dist


def grid_coords(C: int, H: int, W: int, device="cuda") -> torch.Tensor:
    """The fit's own grid as one [(C*H*W),3] device tensor: a trainer constructed on it trains on exactly the coordinates
    a later reconstruction renders (create_coords' values differ from these in the last bit here and there)."""
    spec = GridSpec(C, H, W)
    out = torch.empty(spec.rows, 3, device=device, dtype=torch.float32)
    plane = spec.H * spec.W
    for c0 in range(0, spec.coils_total, MAX_COILS):  # at most 64 coils per description
        sub = GridSpec(C, H, W, coils=list(range(c0, min(c0 + MAX_COILS, spec.coils_total))))
        for lo in range(0, sub.rows, MAX_CALL_ROWS):
            hi = min(lo + MAX_CALL_ROWS, sub.rows)
            grid_rows(sub, lo, hi, coords_out=out[c0 * plane + lo:c0 * plane + hi], with_dist=False)
    return out
