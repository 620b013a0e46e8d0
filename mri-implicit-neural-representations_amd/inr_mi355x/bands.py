"""Radial band statistics (inr_band_stats, csrc/inr_bands.hip): per band of radius, the count, energy,
squared error and extrema of an [n,2] field, in one pass over the data.  It serves the ring statistics of the k-means
partition (clustering.py) and the opt-in per-ring report of the validation epoch, of ``reconstruct --compare`` and of the
ring ensemble.

Row ``i`` belongs to band ``b`` iff ``lo[b] <= dist[i] <= hi[b]``, compared in fp32 with both ends included (a bound is
rounded to fp32 first, as ``(dist >= r0) & (dist <= r1)`` does for an fp32 ``dist``).  Bands may overlap, nest, be empty
or leave rows uncovered; a row on a shared boundary counts in both bands.  With ``mask`` only rows with
``(mask[i] != 0) == (mask_select != 0)`` take part.  Fields, fp64:

    n         rows in the band
    energy    sum of gt_re^2 + gt_im^2
    sse       sum of |pred - gt|^2                               (0 without pred)
    max_abs2  max of fl32(fl32(re*re) + fl32(im*im)) of gt
    max_comp  max of |gt component| over both components
    min_comp  min of |gt component| over both components
    max_err2  max of |pred - gt|^2                               (-inf without pred)

A sum term is formed in fp64 from the fp32 inputs (``dr*dr + di*di`` with ``dr``, ``di`` the fp64 differences, every
operation rounded on its own) and summed in fp64; the extrema are exact.  An empty band has n = 0, sums 0, maxima -inf,
minima +inf.  ``band_stats_numpy`` is this definition in numpy and needs no GPU; the kernel differs from it only in the
order of the fp64 sums.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from .clustering import ring_bounds  # noqa: F401  (re-exported)

FIELDS = ("n", "energy", "sse", "max_abs2", "max_comp", "min_comp", "max_err2")
assert len(FIELDS) == L.BAND_FIELDS
REPORT_HEADERS = ["ring", "lo", "hi", "n", "energy", "err dB", "max |err|"]
REPORT_TITLE = "Per-band error (10 log10(sse / energy))"


class BandStats(NamedTuple):
    lo: np.ndarray  # float32 [K]: the bounds as compared
    hi: np.ndarray
    n: np.ndarray  # float64 [K] each
    energy: np.ndarray
    sse: np.ndarray
    max_abs2: np.ndarray
    max_comp: np.ndarray
    min_comp: np.ndarray
    max_err2: np.ndarray


def _bounds(bounds):
    b = np.asarray(list(bounds), dtype=np.float64).reshape(-1, 2)
    return b[:, 0].astype(np.float32), b[:, 1].astype(np.float32)


def _check_bounds(lo: np.ndarray, hi: np.ndarray) -> None:
    if not 1 <= lo.size <= L.BAND_MAX:
        raise ValueError(f"{lo.size} bands (1..{L.BAND_MAX})")
    if not np.all(lo <= hi):  # NaN too
        raise ValueError("band bounds must be numbers with lo <= hi")


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def band_stats_numpy(dist, gt, pred=None, mask=None, mask_select=1, bounds=()) -> BandStats:
    """The definition above in numpy (float32 comparisons and max_abs2, float64 sums).  Arrays or CPU tensors."""
    as_np = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)
    d = as_np(dist, np.float32).reshape(-1)
    g = as_np(gt, np.float32).reshape(-1, 2)
    p = None if pred is None else as_np(pred, np.float32).reshape(-1, 2)
    lo, hi = _bounds(bounds)
    _check_bounds(lo, hi)
    if g.shape[0] != d.size or (p is not None and p.shape != g.shape):
        raise ValueError(f"dist {d.shape}, gt {g.shape}, pred {None if p is None else p.shape}")
    take = np.ones(d.size, dtype=bool)
    if mask is not None:
        take = (as_np(mask, np.uint8).reshape(-1) != 0) == (int(mask_select) != 0)
    g64 = g.astype(np.float64)
    energy = g64[:, 0] * g64[:, 0] + g64[:, 1] * g64[:, 1]
    abs2 = ((g[:, 0] * g[:, 0]).astype(np.float32) + (g[:, 1] * g[:, 1]).astype(np.float32)).astype(np.float32)
    comp = np.abs(g)
    if p is not None:
        dr, di = p[:, 0].astype(np.float64) - g64[:, 0], p[:, 1].astype(np.float64) - g64[:, 1]
        err2 = dr * dr + di * di
    K = lo.size
    out = {f: np.zeros(K, dtype=np.float64) for f in FIELDS}
    for b in range(K):
        sel = take & (d >= lo[b]) & (d <= hi[b])
        some = bool(sel.any())
        out["n"][b] = float(sel.sum())
        out["energy"][b] = energy[sel].sum(dtype=np.float64)
        out["max_abs2"][b] = float(abs2[sel].max()) if some else -math.inf
        out["max_comp"][b] = float(comp[sel].max()) if some else -math.inf
        out["min_comp"][b] = float(comp[sel].min()) if some else math.inf
        out["sse"][b] = err2[sel].sum(dtype=np.float64) if p is not None else 0.0
        out["max_err2"][b] = float(err2[sel].max()) if (p is not None and some) else -math.inf
    return BandStats(lo, hi, **out)


# ---- the kernel --------------------------------------------------------------------------------------------------------
_scratch = {}  # (n, K, device) -> (stats [K,7] fp64, scratch fp64)


def scratch_doubles(n: int, n_bands: int) -> int:
    out = C.c_int64(0)
    L.check(L.load().inr_band_stats_scratch(int(n), int(n_bands), C.byref(out)))
    return int(out.value)


def _device_input(t: torch.Tensor, name: str, dtype, shape, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: band_stats only runs on an MI355X (no CPU fallback; band_stats_numpy is the "
                           "host-side definition)")
    if t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, dist on {device}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")
    t = t.reshape(shape)
    return t if t.is_contiguous() else t.contiguous()


def band_stats_device(dist, gt, pred=None, mask=None, mask_select=1, bounds=()):
    """One inr_band_stats call on the current stream -> (lo, hi, stats [K,7] fp64 DEVICE tensor, valid until the next
    call with the same (n, K, device)).  Nothing is read back.  Bad bounds (none, more than 64, NaN, lo > hi) raise
    ValueError before anything is allocated."""
    if not isinstance(dist, torch.Tensor) or not dist.is_cuda:
        raise RuntimeError("dist: band_stats only runs on an MI355X (no CPU fallback; band_stats_numpy is the host-side "
                           "definition)")
    device = dist.device
    dist = _device_input(dist, "dist", torch.float32, (-1,), device)
    n = dist.numel()
    gt = _device_input(gt, "gt", torch.float32, (-1, 2), device)
    if pred is not None:
        pred = _device_input(pred, "pred", torch.float32, (-1, 2), device)
    if mask is not None:
        mask = _device_input(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, "mask", torch.uint8, (-1,), device)
    if gt.shape[0] != n or (pred is not None and pred.shape[0] != n) or (mask is not None and mask.numel() != n):
        raise RuntimeError(f"dist has {n} rows, gt {gt.shape[0]}, pred {None if pred is None else pred.shape[0]}, "
                           f"mask {None if mask is None else mask.numel()}")
    lo, hi = _bounds(bounds)
    _check_bounds(lo, hi)  # (the library checks again; its buffers are sized from K here)
    if n < 1:
        raise ValueError("band_stats of no rows")
    K = int(lo.size)
    key = (n, K, device)
    if key not in _scratch:
        _scratch[key] = (torch.empty(K, L.BAND_FIELDS, device=device, dtype=torch.float64),
                         torch.empty(scratch_doubles(n, K), device=device, dtype=torch.float64))
    stats, scratch = _scratch[key]
    FP = C.POINTER(C.c_float)
    L.launch("inr_band_stats", device, dist.data_ptr(), gt.data_ptr(), None if pred is None else pred.data_ptr(),
             None if mask is None else mask.data_ptr(), int(mask_select), n, lo.ctypes.data_as(FP), hi.ctypes.data_as(FP),
             K, stats.data_ptr(), scratch.data_ptr())
    return lo, hi, stats


def _from_rows(lo, hi, rows: np.ndarray) -> BandStats:
    return BandStats(lo, hi, *(np.ascontiguousarray(rows[:, f]) for f in range(L.BAND_FIELDS)))


def band_stats(dist, gt, pred=None, mask=None, mask_select=1, bounds=()) -> BandStats:
    """Device tensors -> BandStats on the host: one launch sequence, one read-back of K x 7 doubles."""
    lo, hi, stats = band_stats_device(dist, gt, pred, mask, mask_select, bounds)
    return _from_rows(lo, hi, stats.cpu().numpy())


def band_stats_many(dist, gt, pred, selections, bounds) -> list:
    """One BandStats per (mask, mask_select) of ``selections`` with ONE read-back for all of them."""
    parts, lo, hi = [], None, None
    for mask, sel in selections:
        lo, hi, stats = band_stats_device(dist, gt, pred, mask, sel, bounds)
        parts.append(stats.clone())  # the cached output buffer is reused by the next call
    host = torch.stack(parts).cpu().numpy()
    return [_from_rows(lo, hi, host[k]) for k in range(len(parts))]


# ---- the report --------------------------------------------------------------------------------------------------------
def band_report(stats: BandStats) -> list:
    """[{lo, hi, n, energy, sse, err_db, max_abs_err}] per band: err_db = 10 log10(sse / energy), None where the band is
    empty or carries no energy (-inf for an exact fit); max_abs_err = sqrt(max_err2), None without rows or prediction."""
    out = []
    for b in range(len(stats.lo)):
        n, energy, sse, me2 = int(stats.n[b]), float(stats.energy[b]), float(stats.sse[b]), float(stats.max_err2[b])
        if n == 0 or energy == 0.0:
            err_db = None
        else:
            err_db = 10.0 * math.log10(sse / energy) if sse > 0.0 else -math.inf
        out.append({"lo": float(stats.lo[b]), "hi": float(stats.hi[b]), "n": n, "energy": energy, "sse": sse,
                    "err_db": err_db, "max_abs_err": math.sqrt(me2) if (n > 0 and me2 >= 0.0) else None})
    return out


def format_band_table(report, title: str = REPORT_TITLE) -> str:
    """The report as text, laid out like the per-coil table (display.coil_stats_table): title line, then tabulate's
    table, or a fixed-width table of the same numbers when tabulate is not installed."""
    cell = lambda v: "n/a" if v is None else "%.6g" % v
    rows = [[str(i), cell(r["lo"]), cell(r["hi"]), str(r["n"]), cell(r["energy"]), cell(r["err_db"]),
             cell(r["max_abs_err"])] for i, r in enumerate(report)]
    try:
        from tabulate import tabulate
        table = tabulate(rows, headers=REPORT_HEADERS, disable_numparse=True, stralign="right")
    except ImportError:
        cells = [REPORT_HEADERS] + rows
        k_n = len(REPORT_HEADERS)
        widths = [max(len(c[k]) for c in cells) + (2 if k else 0) for k in range(k_n)]
        lines = ["".join(c[k].rjust(widths[k]) for k in range(k_n)) for c in cells]
        lines.insert(1, "".join(("-" * (widths[k] - (2 if k else 0))).rjust(widths[k]) for k in range(k_n)))
        table = "\n".join(lines)
    return "{}\n{}".format(title, table)


def report_bounds(arg, default_steps: int = 40):
    """Bounds of a report from what the caller gave: None -> ring_bounds(default_steps), an int N -> ring_bounds(N), else
    the (lo, hi) pairs themselves."""
    if arg is None or arg is True:
        out = ring_bounds(default_steps)
    elif isinstance(arg, (int, np.integer)):
        out = ring_bounds(int(arg))
    else:
        out = [(float(a), float(b)) for a, b in arg]
    _check_bounds(*_bounds(out))  # ValueError here, not inside the first validation
    return out


def _rings_argument(text: str) -> int:
    """N of --band-report N: the one place its range is checked"""
    import argparse
    try:
        n = int(text)
    except ValueError:
        n = 0
    if not 1 <= n <= L.BAND_MAX:
        raise argparse.ArgumentTypeError(f"{text!r}: a number of rings, 1..{L.BAND_MAX}")
    return n


def add_band_report_flag(ap, needs: str) -> None:
    """--band-report [N] -> opts.band_report: None (absent), 0 (no N: the default rings) or N in 1..64"""
    ap.add_argument("--band-report", type=_rings_argument, nargs="?", const=0, default=None, metavar="N",
                    help=f"{needs}: error by radius, 10 log10(sse / energy) per ring of k-space, as a table and in the "
                         "JSON result; N rings (default: the config's partition no_steps, else 40)")


def flag_bounds(value):
    """--band-report's value -> the ``bounds`` argument of enable_band_report / compare (None: not asked for)."""
    if value is None:
        return None
    return True if value == 0 else int(value)
