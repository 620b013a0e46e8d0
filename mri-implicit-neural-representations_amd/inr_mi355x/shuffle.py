"""Shuffled epochs: a keyed, stateless permutation of the rows and the host side of the kernel
that applies it on the device (inr_shuffle_epoch).

``epoch_order(n, seed, epoch)`` is the specification restated in numpy: a pure function of its arguments (no generator
state), so a resumed fit continues with the order it would have had and every data-parallel rank derives the same order
without communication.  The kernel computes the same integers in registers; the two agree bit for bit.

The reference has no counterpart beyond the ``shuffle=True`` its callers pass and its loaders drop
(train.py:281,307 against models/utils.py:84-99).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

ROUNDS = 6
GOLD = 0x9E3779B9
_M32 = 0xFFFFFFFF
MAX_ROWS = 1 << 31


def _mix(x: int) -> int:
    """MIX of section 4.12 on one Python int (the key schedule)."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def _mix_np(x: np.ndarray) -> np.ndarray:
    """MIX on a uint32 array (products wrap modulo 2^32)."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def domain_bits(n: int) -> int:
    """k: the smallest even k >= 8 with 2^k >= n (a balanced Feistel network needs two halves of k / 2 bits; 8 bits at
    least so that tiny n -- the 15 coils of a per-coil fit -- still draw from a domain with many permutations)."""
    k = 8
    while (1 << k) < n:
        k += 2
    return k


def round_keys(seed: int, epoch: int) -> List[int]:
    """The ROUNDS 32-bit round keys of (seed, epoch): seed is taken modulo 2^64, epoch modulo 2^32."""
    seed &= (1 << 64) - 1
    base = _mix(_mix(_mix((seed & _M32) + GOLD) ^ (seed >> 32)) + (epoch & _M32))
    return [_mix(base + (r + 1) * GOLD) for r in range(ROUNDS)]


def _check_n(n: int) -> int:
    n = int(n)
    if n < 1:
        raise ValueError(f"epoch_order: n = {n}")
    if n >= MAX_ROWS:
        raise ValueError(f"epoch_order: n = {n} rows; the 32-bit permutation covers n < 2^31")
    return n


def epoch_order(n: int, seed: int, epoch: int) -> np.ndarray:
    """order[j] = the row that sits at position j of epoch ``epoch``: int64 [n], a permutation of range(n)."""
    n = _check_n(n)
    keys = [np.uint32(k) for k in round_keys(int(seed), int(epoch))]
    h = np.uint32(domain_bits(n) // 2)
    half = np.uint32((1 << int(h)) - 1)

    def permute(x):
        left, right = x >> h, x & half
        for k in keys:
            left, right = right, left ^ ((_mix_np(right ^ k) >> np.uint32(16)) & half)
        return (left << h) | right

    with np.errstate(over="ignore"):
        out = permute(np.arange(n, dtype=np.uint32))
        todo = np.nonzero(out >= n)[0]
        while todo.size:  # cycle walking: a point that left [0, n) goes through the bijection again
            out[todo] = permute(out[todo])
            todo = todo[out[todo] >= n]
    return out.astype(np.int64)


def coil_order(n_coils: int, seed: int, epoch: int) -> List[int]:
    """Per-coil fits keep their batches (one coil = one view of the resident grid) and visit them in this order."""
    return epoch_order(n_coils, seed, epoch).tolist()


class CoilOrder:
    """coil_order of the current epoch, kept until the epoch changes."""

    def __init__(self, n_coils: int, seed: int):
        self.n_coils, self.seed, self.epoch, self.order = int(n_coils), int(seed), None, None

    def at(self, epoch: int, it: int) -> int:
        if epoch != self.epoch:
            self.epoch, self.order = epoch, coil_order(self.n_coils, self.seed, epoch)
        return self.order[it]


def shuffle_settings(config: dict, seed: int, graph_steps: bool = False):
    """(shuffle, shuffle_seed) of a trainer config; ``shuffle_seed`` defaults to the trainer's seed.  Captured steps
    bake a batch's count and views, so ``graph_steps`` with ``shuffle`` is refused rather than one of them ignored."""
    on = bool(config.get("shuffle", False))
    if on and graph_steps:
        raise ValueError("shuffle with graph_steps: a captured step bakes its batch's views and count; pick one")
    s = config.get("shuffle_seed")
    return on, int(seed if s is None else s)


def _dev(t: Optional[torch.Tensor], name: str, dtype, shape: Sequence[int], device=None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the INR engine only runs on an MI355X (no CPU fallback)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, the other buffers on {device}")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.data_ptr()


def shuffle_epoch(n: int, seed: int, epoch: int, device, *, coords=None, coords_out=None, gt=None, gt_out=None,
                  dist=None, dist_out=None, mask=None, mask_out=None, batch_size: int = 0, batch_counts=None,
                  order_out=None) -> None:
    """inr_shuffle_epoch on the current stream: every ``x_out[j] = x[order[j]]`` for the pairs given, ``batch_counts[b]``
    (int32, ceil(n / batch_size) entries) = sampled rows among output rows [b*bs, (b+1)*bs), ``order_out`` (int64 [n]) =
    the order itself.  The caller owns every buffer; nothing is allocated and nothing is read back here."""
    n = _check_n(n)
    device = torch.device(device)
    if device.index is None and device.type == "cuda":
        device = torch.device("cuda", torch.cuda.current_device())
    for a, b, name in ((coords, coords_out, "coords"), (gt, gt_out, "gt"), (dist, dist_out, "dist"),
                       (mask, mask_out, "mask")):
        if (a is None) != (b is None) and not (name == "mask" and b is None):
            raise RuntimeError(f"{name} and {name}_out go together")
    nb = 0
    if batch_counts is not None:
        if batch_size < 1:
            raise RuntimeError(f"batch_counts needs batch_size >= 1 (got {batch_size})")
        nb = -(-n // int(batch_size))
    ptrs = [_dev(coords, "coords", torch.float32, (n, 3), device), _dev(gt, "gt", torch.float32, (n, 2), device),
            _dev(dist, "dist", torch.float32, (n,), device), _dev(mask, "mask", torch.uint8, (n,), device),
            _dev(coords_out, "coords_out", torch.float32, (n, 3), device),
            _dev(gt_out, "gt_out", torch.float32, (n, 2), device),
            _dev(dist_out, "dist_out", torch.float32, (n,), device),
            _dev(mask_out, "mask_out", torch.uint8, (n,), device),
            _dev(batch_counts, "batch_counts", torch.int32, (nb,), device),
            _dev(order_out, "order_out", torch.int64, (n,), device)]
    L.check(L.load().inr_shuffle_epoch(n, int(batch_size), C.c_uint64(int(seed) & ((1 << 64) - 1)),
                                       C.c_uint32(int(epoch) & _M32), *ptrs,
                                       torch.cuda.current_stream(device).cuda_stream))


def device_order(n: int, seed: int, epoch: int, device) -> torch.Tensor:
    """The epoch's order as an int64 device tensor (what ``epoch_order`` gives, made by the kernel)."""
    out = torch.empty(n, dtype=torch.int64, device=device)
    shuffle_epoch(n, seed, epoch, device, order_out=out)
    return out


class EpochBuffers:
    """The second set of resident buffers a shuffled fit trains from: the epoch's copies of coords / image (/ dist / mask)
    and its per-batch sampled-row counts.  ``begin(epoch)`` is one kernel launch and ONE small device-to-host copy (the
    counts); a repeated call for the epoch already held does nothing."""

    def __init__(self, seed: int, batch_size: int, coords: torch.Tensor, image: torch.Tensor,
                 dist: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        self.seed, self.bs, self.n = int(seed), int(batch_size), int(coords.shape[0])
        _check_n(self.n)
        self.src = (coords, image, dist, mask)
        self.coords, self.image = torch.empty_like(coords), torch.empty_like(image)
        self.dist = None if dist is None else torch.empty_like(dist)
        self.mask = None if mask is None else torch.empty_like(mask)
        self.n_batches = -(-self.n // self.bs)
        self._counts_dev = torch.empty(self.n_batches, dtype=torch.int32, device=coords.device)
        self.counts: List[int] = []
        self.epoch = None

    def begin(self, epoch: int) -> bool:
        """True when the buffers were refilled (the caller recomputes what it derives from a batch's contents)."""
        if epoch == self.epoch:
            return False
        coords, image, dist, mask = self.src
        shuffle_epoch(self.n, self.seed, epoch, coords.device, coords=coords, coords_out=self.coords, gt=image,
                      gt_out=self.image, dist=dist, dist_out=self.dist, mask=mask, mask_out=self.mask,
                      batch_size=self.bs, batch_counts=self._counts_dev)
        self.counts = self._counts_dev.tolist()
        self.epoch = epoch
        return True

    def batch_sums(self, flags: torch.Tensor) -> torch.Tensor:
        """Per-batch sums of ``flags`` [..., n] (bool / integer) over the batches of the epoch buffer: int64 [..., n_batches]
        on the device, one batched op (a cumulative sum cut at the batch ends)."""
        cum = torch.cumsum(flags.to(torch.int64), dim=-1)
        ends = torch.arange(1, self.n_batches + 1, device=flags.device).mul_(self.bs).clamp_(max=self.n) - 1
        at = cum.index_select(-1, ends)
        return torch.diff(at, dim=-1, prepend=torch.zeros_like(at[..., :1]))

    def batch_means(self, values: torch.Tensor) -> List[float]:
        """Per-batch means of ``values`` [n] (fp32), each taken by torch.mean over the batch's rows: one read-back."""
        full = self.n // self.bs
        parts = []
        if full:
            parts.append(values[:full * self.bs].view(full, self.bs).mean(dim=1))
        if full * self.bs < self.n:
            parts.append(values[full * self.bs:].mean().reshape(1))
        return torch.cat(parts).tolist()
