"""Weighted epochs: the rows of an epoch drawn with probability proportional to a per-row
weight, and the host side of the two kernels that do it on the device (inr_row_cdf, inr_sample_epoch;
csrc/inr_sample.hip).

Drawing row ``i`` with probability ``w_i / sum w`` makes the expected gradient of the UNWEIGHTED step that of the weighted
loss ``sum w_i l_i / sum w_i`` -- so no fused kernel takes a weight argument; the feature is a second way to fill the
epoch buffers the trainers already train from (shuffle.EpochBuffers).

The definition, integer arithmetic after one fp64 product per row:

* ticks: ``q_i = 0`` where ``mask[i] == 0`` or ``w_i`` is NaN, negative or +-0; otherwise
  ``min(2^32 - 1, floor(fp64(w_i) * scale))`` (``+inf`` gives ``2^32 - 1``).  ``cdf[i] = q_0 + ... + q_i`` as uint64.
* draw of ``m`` rows: with ``T = cdf[n-1]`` and ``stride = T // m``, position ``j`` holds stratum
  ``s = epoch_order(m, seed, epoch)[j]``; its threshold is ``t_s = s * stride + (u_s mod stride)`` with
  ``u_s = MIX(s ^ k0) * 2^32 + MIX(s ^ k1)`` under ``draw_keys(seed, epoch)``; the row is the smallest ``i`` with
  ``cdf[i] > t_s``.  One threshold per stratum of ``stride`` ticks (stratified, low variance); stateless like the shuffle:
  a resumed fit and every rank derive the same draw.

``row_ticks_numpy`` / ``row_cdf_numpy`` / ``epoch_draw_numpy`` are this definition in numpy and need no GPU; the kernels
give the same integers bit for bit.  What follows from it: a row without ticks is never drawn; row ``i`` is drawn between
``max(0, q_i // stride - 1)`` and ``q_i // stride + 2`` times, provided ``T mod m < stride`` (the strata cover
``[0, m * stride)``: the last ``T mod m`` ticks are never reached -- with the default scale a share below ``m / 2^32`` of
the heaviest row); equal ticks and ``m == n`` give ``epoch_order(n, seed, epoch)`` itself.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from .shuffle import _M32, MAX_ROWS, EpochBuffers, _dev, _mix, _mix_np, epoch_order

MAX_TICKS = (1 << 32) - 1
DRAW_CONSTANT = 0x85EBCA6B
MODES = ("uniform", "density", "ring-inverse")


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def default_scale(w_max: float) -> float:
    """the scale under which the heaviest row gets 2^32 - 1 ticks"""
    return float(MAX_TICKS) / float(w_max)


def _check_scale(scale) -> float:
    scale = float(scale)
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"scale = {scale!r} (must be finite and > 0)")
    return scale


def _check_rows(v: int, name: str) -> int:
    v = int(v)
    if v < 1 or v >= MAX_ROWS:
        raise ValueError(f"{name} = {v} (1 <= {name} < 2^31)")
    return v


def row_ticks_numpy(w, scale: float, mask=None) -> np.ndarray:
    """uint64 [n]: the ticks of every row (each <= 2^32 - 1)"""
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))
    scale = _check_scale(scale)
    live = w > 0  # False for NaN, negatives and both zeros
    if mask is not None:
        m = np.asarray(mask).reshape(-1)
        if m.shape != w.shape:
            raise ValueError(f"mask has {m.size} rows, w {w.size}")
        live &= m != 0
    q = np.zeros(w.shape, dtype=np.uint64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.floor(w[live].astype(np.float64) * np.float64(scale))  # one product, rounded once
    q[live] = np.minimum(p, float(MAX_TICKS)).astype(np.uint64)
    return q


def row_cdf_numpy(w, scale: float, mask=None) -> np.ndarray:
    """uint64 [n]: the inclusive sums of row_ticks_numpy"""
    q = row_ticks_numpy(w, scale, mask)
    _check_rows(q.size, "n")
    return np.cumsum(q, dtype=np.uint64)


def draw_keys(seed: int, epoch: int) -> List[int]:
    """The two 32-bit keys of a stratum's offset: shuffle.round_keys' schedule under another constant."""
    seed &= (1 << 64) - 1
    base = _mix(_mix(_mix((seed & _M32) + DRAW_CONSTANT) ^ (seed >> 32)) + (epoch & _M32))
    return [_mix(base + (r + 1) * DRAW_CONSTANT) for r in range(2)]


def epoch_draw_numpy(cdf, m: int, seed: int, epoch: int) -> np.ndarray:
    """int64 [m]: the row at every position of epoch ``epoch``'s draw from ``cdf`` (uint64 [n], non-decreasing)."""
    cdf = np.ascontiguousarray(np.asarray(cdf).reshape(-1)).astype(np.uint64, copy=False)
    n, m = _check_rows(cdf.size, "n"), _check_rows(m, "m")
    total = int(cdf[n - 1])
    if total == 0:
        return np.zeros(m, dtype=np.int64)
    stride = total // m
    t = np.zeros(m, dtype=np.uint64)
    if stride:
        s = epoch_order(m, seed, epoch).astype(np.uint32)
        k0, k1 = (np.uint32(k) for k in draw_keys(int(seed), int(epoch)))
        with np.errstate(over="ignore"):
            u = (_mix_np(s ^ k0).astype(np.uint64) << np.uint64(32)) | _mix_np(s ^ k1).astype(np.uint64)
        t = s.astype(np.uint64) * np.uint64(stride) + u % np.uint64(stride)
    return np.searchsorted(cdf, t, side="right").astype(np.int64)  # the smallest i with cdf[i] > t: < n, as t < total


# ---- the kernels -------------------------------------------------------------------------------------------------------
@dataclass
class RowCdf:
    cdf: torch.Tensor  # int64 [n] on the device: the uint64 sums (below 2^63 for n < 2^31, so the same bits)
    scale: float
    total_ticks: int
    zero_weight_rows: int

    @property
    def n(self) -> int:
        return int(self.cdf.numel())


def _device_weights(w, n: Optional[int] = None) -> torch.Tensor:
    if not isinstance(w, torch.Tensor) or not w.is_cuda:
        raise RuntimeError("weights: row_cdf only runs on an MI355X (no CPU fallback; row_cdf_numpy is the host-side "
                           "definition)")
    if w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous():
        raise RuntimeError(f"weights must be a contiguous torch.float32 [n] tensor (got {w.dtype} {tuple(w.shape)})")
    if n is not None and w.numel() != n:
        raise ValueError(f"{w.numel()} weights for {n} rows")
    return w


def row_cdf(w: torch.Tensor, mask: Optional[torch.Tensor] = None, scale: Optional[float] = None,
            rows: Optional[int] = None) -> RowCdf:
    """inr_row_cdf on the current stream: the CDF a draw of ``rows`` (default n) rows reads.  ``scale`` None:
    default_scale of the largest finite weight among the rows that can be drawn, read back from the device (the scale is
    a host argument of the call).  One more read-back brings the total and the number of rows without ticks.  ValueError
    when no row has ticks, when the total is below ``rows`` (stride 0), or for a scale that is not finite and positive."""
    w = _device_weights(w)
    n = _check_rows(w.numel(), "n")
    m = n if rows is None else _check_rows(rows, "rows")
    mask_ptr = _dev(mask, "mask", torch.uint8, (n,), w.device)
    if scale is None:
        ok = torch.isfinite(w) & (w > 0)
        if mask is not None:
            ok &= mask != 0
        w_max = float(torch.where(ok, w, torch.zeros_like(w)).max())
        if not w_max > 0.0:
            raise ValueError("row_cdf: no row has a positive finite weight" + (" under the mask" if mask is not None else ""))
        scale = default_scale(w_max)
    scale = _check_scale(scale)
    lib = L.load()
    words = C.c_int64(0)
    L.check(lib.inr_row_cdf_scratch(n, C.byref(words)))
    cdf = torch.empty(n, dtype=torch.int64, device=w.device)
    scratch = torch.empty(words.value, dtype=torch.int64, device=w.device)
    L.launch("inr_row_cdf", w.device, w.data_ptr(), mask_ptr, n, C.c_double(scale), cdf.data_ptr(), scratch.data_ptr(),
             words.value)
    zero = (cdf[1:] == cdf[:-1]).sum() + (cdf[0] == 0)
    total, zero = torch.stack((cdf[n - 1], zero)).tolist()
    if total == 0:
        raise ValueError(f"row_cdf: no row has ticks at scale {scale:g}")
    if total < m:
        raise ValueError(f"row_cdf: {total} ticks in all for a draw of {m} rows (stride 0): raise the scale")
    return RowCdf(cdf, scale, int(total), int(zero))


def sample_epoch(cdf: torch.Tensor, m: int, seed: int, epoch: int, *, coords=None, coords_out=None, gt=None, gt_out=None,
                 dist=None, dist_out=None, mask=None, mask_out=None, batch_size: int = 0, batch_counts=None,
                 order_out=None) -> None:
    """inr_sample_epoch on the current stream: every ``x_out[j] = x[row(j)]`` for the pairs given (inputs of n rows,
    outputs of ``m``), ``batch_counts[b]`` (int32, ceil(m / batch_size) entries) = sampled rows among output rows
    [b*bs, (b+1)*bs), ``order_out`` (int64 [m]) = the draw itself.  The caller owns every buffer; nothing is allocated
    and nothing is read back here."""
    if not isinstance(cdf, torch.Tensor) or not cdf.is_cuda or cdf.dtype != torch.int64 or cdf.dim() != 1 \
            or not cdf.is_contiguous():
        raise RuntimeError("cdf must be a contiguous int64 [n] device tensor (RowCdf.cdf)")
    n, m, device = _check_rows(cdf.numel(), "n"), _check_rows(m, "m"), cdf.device
    for a, b, name in ((coords, coords_out, "coords"), (gt, gt_out, "gt"), (dist, dist_out, "dist"),
                       (mask, mask_out, "mask")):
        if (a is None) != (b is None) and not (name == "mask" and b is None):
            raise RuntimeError(f"{name} and {name}_out go together")
    nb = 0
    if batch_counts is not None:
        if batch_size < 1:
            raise RuntimeError(f"batch_counts needs batch_size >= 1 (got {batch_size})")
        nb = -(-m // int(batch_size))
    ptrs = [_dev(coords, "coords", torch.float32, (n, 3), device), _dev(gt, "gt", torch.float32, (n, 2), device),
            _dev(dist, "dist", torch.float32, (n,), device), _dev(mask, "mask", torch.uint8, (n,), device),
            _dev(coords_out, "coords_out", torch.float32, (m, 3), device),
            _dev(gt_out, "gt_out", torch.float32, (m, 2), device),
            _dev(dist_out, "dist_out", torch.float32, (m,), device),
            _dev(mask_out, "mask_out", torch.uint8, (m,), device),
            _dev(batch_counts, "batch_counts", torch.int32, (nb,), device),
            _dev(order_out, "order_out", torch.int64, (m,), device)]
    L.launch("inr_sample_epoch", device, cdf.data_ptr(), n, m, int(batch_size), C.c_uint64(int(seed) & ((1 << 64) - 1)),
             C.c_uint32(int(epoch) & _M32), *ptrs)


def device_draw(cdf: torch.Tensor, m: int, seed: int, epoch: int) -> torch.Tensor:
    """The epoch's draw as an int64 device tensor (what ``epoch_draw_numpy`` gives, made by the kernel)."""
    out = torch.empty(int(m), dtype=torch.int64, device=cdf.device)
    sample_epoch(cdf, m, seed, epoch, order_out=out)
    return out


class WeightedEpochBuffers(EpochBuffers):
    """shuffle.EpochBuffers filled by a weighted draw: ``rows`` (default n) rows per epoch, drawn from ``weights`` (device
    fp32 [n]; rows with mask == 0 get no ticks, so every drawn row is a sampled one).  ``begin(epoch)`` is one kernel launch
    and one small read-back, as there; ``set_weights`` replaces the CDF and takes effect at the next refill."""

    def __init__(self, seed: int, batch_size: int, weights: torch.Tensor, coords: torch.Tensor, image: torch.Tensor,
                 dist: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, rows: Optional[int] = None,
                 mode: str = "weights"):
        self.seed, self.bs, self.n_src = int(seed), int(batch_size), _check_rows(coords.shape[0], "n")
        self.n = self.n_src if rows is None else _check_rows(rows, "rows")  # the rows of the buffers, as in EpochBuffers
        self.mode = mode
        self.src = (coords, image, dist, mask)
        self.set_weights(weights)
        self.coords, self.image = coords.new_empty((self.n, 3)), image.new_empty((self.n, 2))
        self.dist = None if dist is None else dist.new_empty(self.n)
        self.mask = None if mask is None else mask.new_empty(self.n)
        self.n_batches = -(-self.n // self.bs)
        self._counts_dev = torch.empty(self.n_batches, dtype=torch.int32, device=coords.device)
        self.counts: List[int] = []
        self.epoch = None

    def set_weights(self, weights: torch.Tensor) -> None:
        self.row_cdf = row_cdf(_device_weights(weights, self.n_src), self.src[3], rows=self.n)

    def draw(self, epoch: int) -> torch.Tensor:
        """int64 [rows]: the source row at every position of epoch ``epoch`` under the current weights"""
        return device_draw(self.row_cdf.cdf, self.n, self.seed, epoch)

    def begin(self, epoch: int) -> bool:
        if epoch == self.epoch:
            return False
        coords, image, dist, mask = self.src
        sample_epoch(self.row_cdf.cdf, self.n, self.seed, epoch, coords=coords, coords_out=self.coords, gt=image,
                     gt_out=self.image, dist=dist, dist_out=self.dist, mask=mask, mask_out=self.mask,
                     batch_size=self.bs, batch_counts=self._counts_dev)
        self.counts = self._counts_dev.tolist()
        self.epoch = epoch
        return True

    def summary(self) -> dict:
        """what the JSON result, metrics() and the validation records carry"""
        return {"mode": self.mode, "rows": self.n, "zero_weight_rows": self.row_cdf.zero_weight_rows,
                "total_ticks": self.row_cdf.total_ticks}


# ---- config key, weights and command line ------------------------------------------------------------------------------
def parse_row_sampling(arg) -> Optional[str]:
    """config['row_sampling']: None (off) | 'uniform' | 'density' | 'ring-inverse' | the path of a FILE.npy"""
    if arg is None or arg is False:
        return None
    if not isinstance(arg, str):
        raise ValueError(f"row_sampling = {arg!r}: none | uniform | density | ring-inverse | FILE.npy")
    if arg.lower() == "none":
        return None
    if arg in MODES:
        return arg
    if arg.endswith(".npy"):
        if not os.path.isfile(arg):
            raise ValueError(f"row_sampling = {arg!r}: no such file")
        return arg
    raise ValueError(f"row_sampling = {arg!r}: none | uniform | density | ring-inverse | FILE.npy")


def check_row_sampling(config: dict, trajectory, graph_steps: bool, world: int) -> Optional[str]:
    """The parsed key, after refusing what a weighted epoch cannot be combined with -- before anything is allocated."""
    spec = parse_row_sampling(config.get("row_sampling"))
    if spec is None:
        return None
    if graph_steps:
        raise ValueError(f"row_sampling = {spec!r} with graph_steps: a captured step bakes its batch's views and count; "
                         "pick one")
    if config.get("per_coil") or config.get("use_tv"):
        raise ValueError(f"row_sampling = {spec!r} with per_coil / use_tv: drawn rows do not form a coil grid")
    if config.get("loss") == "LSL":
        raise NotImplementedError(f"row_sampling = {spec!r} with loss 'LSL' (CenterLoss)")
    if world > 1:
        raise NotImplementedError(f"row_sampling = {spec!r} on more than one rank")
    if spec == "density" and trajectory is None:
        raise ValueError("row_sampling = 'density' without config['trajectory']: the density weights belong to off-grid "
                         "samples")
    return spec


def file_weights(path: str, n: int) -> np.ndarray:
    """fp32 [n] from a .npy file of [n] finite, non-negative fp32 or fp64"""
    w = np.load(path, allow_pickle=False)
    if w.dtype not in (np.float32, np.float64) or w.shape != (n,) or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"row_sampling = {path!r}: expected [{n}] finite non-negative float32 / float64, got {w.dtype} "
                         f"{w.shape}")
    return w.astype(np.float32)


def density_weights(trajectory, coils: int, H: int, W: int, density=None) -> np.ndarray:
    """fp32 [coils * M]: trajectory.parse_density's weights (config['trajectory_density'], default ramp) repeated per coil
    in the row order of trajectory.trajectory_coords (coil-major)"""
    from .trajectory import parse_density
    if trajectory is None:
        raise ValueError("row_sampling = 'density' needs a trajectory")
    w = parse_density(density, trajectory, int(H), int(W))[1]
    return np.tile(w.astype(np.float32), int(coils))


def _open_table(radii, divisors):
    """the table with its outer ends opened, so that every row with a radius lies in a ring"""
    r = np.asarray(radii, dtype=np.float64).copy()
    r[0], r[-1] = -np.inf, np.inf
    return r, np.asarray(divisors, dtype=np.float32)


def ring_inverse_weights_numpy(dist, radii, divisors) -> np.ndarray:
    """fp32 [n]: fl32(fl32(1 / divisor[r]) * divisor[last]) for a row in ring r (the first and last ring reach to -inf and
    +inf) -- the reference's stats_rec (train_variations/train_weighted_kspace.py:110-115) per row"""
    from .ringnorm import ring_scale_numpy
    r, d = _open_table(radii, divisors)
    n = np.asarray(dist).reshape(-1).size
    inv = ring_scale_numpy(dist, np.ones((n, 2), dtype=np.float32), r, d)[:, 0]
    return (inv * d[-1]).astype(np.float32)


def ring_inverse_weights(values: torch.Tensor, dist: torch.Tensor, no_steps: int = 40, no_models: int = 4) -> torch.Tensor:
    """The same on the device, from the RingTable.from_rows(..., 'max') of the training rows themselves: one
    inr_ring_scale call on a column of ones.  Sampling with these weights equals, in expectation, that script's per-row
    loss weighting; its per-ring means and the optimizer step inside its ring loop are not reproduced."""
    from .ringnorm import RingTable, ring_scale
    table = RingTable.from_rows(values, dist, no_steps, no_models, "max")
    r, d = _open_table(table.radii, table.divisors)
    inv = ring_scale(dist, torch.ones_like(values), r, d)[:, 0]
    return (inv * float(d[-1])).contiguous()


def make_weights(spec: str, config: dict, coords: torch.Tensor, values: torch.Tensor, shape, trajectory=None) -> torch.Tensor:
    """The device fp32 [n] weights of a parsed config['row_sampling'] for the training rows (coords [n,3], values [n,2])"""
    n, device = int(coords.shape[0]), coords.device
    if spec == "uniform":
        return torch.ones(n, dtype=torch.float32, device=device)
    if spec == "density":
        w = density_weights(trajectory, int(shape[0]), int(shape[1]), int(shape[2]), config.get("trajectory_density"))
        if w.size != n:
            raise ValueError(f"row_sampling = 'density': {w.size} weights for {n} training rows")
        return torch.from_numpy(w).to(device)
    if spec == "ring-inverse":
        from .ringnorm import partition_counts
        dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2).contiguous()
        return ring_inverse_weights(values, dist, *partition_counts(config))
    return torch.from_numpy(file_weights(spec, n)).to(device)


def add_row_sampling_flag(ap) -> None:
    ap.add_argument("--row-sampling", type=str, default=None, metavar="ARG",
                    help="python -m inr_mi355x.train only (the other drivers refuse it): draw every epoch's rows with "
                         "probability proportional to a per-row weight: uniform | density (needs --trajectory) | "
                         "ring-inverse | FILE.npy of [n_train] weights (config['row_sampling']; none: off)")


def apply_row_sampling_flag(config: dict, opts) -> dict:
    if getattr(opts, "row_sampling", None) is not None:
        config["row_sampling"] = opts.row_sampling
    return config
