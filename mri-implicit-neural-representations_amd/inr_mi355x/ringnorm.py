"""Ring-normalised fits (inr_ring_scale, csrc/inr_ring_scale.hip): k-space is partitioned into rings by
k-means, every ring is divided by its summary statistic before the fit and multiplied back before anything is scored
(the reference's src/train_variations/train_normalize_per_bucket.py:20-27,131,142-150,213).

The scaling.  Row ``i`` belongs to ring ``r`` iff ``radii[r] <= dist[i] < radii[r+1]``, compared in fp32 with the lower
end included and the upper end excluded (the radii are rounded to fp32 first).  Both components of such a row become
``in / divisors[r]``, one correctly rounded fp32 division each.  A row in no ring -- ``dist`` below ``radii[0]``, at or
above the last radius, NaN -- is copied unchanged, bit for bit.  Equal neighbouring radii make an empty ring; a row at
that radius falls into the next non-empty one.  The inverse is the same call with the table ``fl32(1 / divisors[r])``
(``inverse_divisors``), as the reference's ``stats_rec`` is: there is no second code path.  ``ring_scale_numpy`` is this
definition in numpy and needs no GPU; ``ring_scale`` is the kernel.

Two interval conventions meet here, on purpose.  The STATISTICS of a ring (``RingTable.from_rows``) use closed intervals
``radii[r] <= dist <= radii[r+1]``, as clustering.partition_and_stats and the reference's clustering.py:100-135 do: a row
exactly on a shared radius counts in the statistics of both neighbours.  The SCALING uses the half-open intervals above,
as the reference's scale_space does: such a row is divided by the outer neighbour's divisor only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L

STATS = ("max", "min")


def _table(radii, divisors):
    """(radii fp32 [K+1], divisors fp32 [K]) as compared and divided by, checked as the library checks them"""
    r = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1).astype(np.float32))
    d = np.ascontiguousarray(np.asarray(divisors, dtype=np.float32).reshape(-1))
    if not 1 <= d.size <= L.BAND_MAX:
        raise ValueError(f"{d.size} rings (1..{L.BAND_MAX})")
    if r.size != d.size + 1:
        raise ValueError(f"{r.size} radii for {d.size} divisors (a table of K rings has K + 1 radii)")
    if np.isnan(r).any() or np.any(r[1:] < r[:-1]):
        raise ValueError("radii must be numbers that do not decrease")
    if not np.all(np.isfinite(d)) or np.any(d == 0):
        raise ValueError("divisors must be finite and not zero")
    return r, d


def inverse_divisors(divisors) -> np.ndarray:
    """fl32(1 / d) per ring: the table of the inverse scaling (train_normalize_per_bucket.py:131)"""
    d = np.asarray(divisors, dtype=np.float32)
    return (np.float32(1.0) / d).astype(np.float32)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def ring_scale_numpy(dist, values, radii, divisors) -> np.ndarray:
    """The definition above in numpy: [n,2] fp32.  Arrays or CPU tensors; the input is not modified."""
    as_np = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
    d = as_np(dist).reshape(-1)
    v = as_np(values).reshape(-1, 2)
    r32, d32 = _table(radii, divisors)
    if v.shape[0] != d.size:
        raise ValueError(f"dist has {d.size} rows, values {v.shape[0]}")
    ring = np.searchsorted(r32, d, side="right") - 1  # NaN sorts behind every radius: ring K, outside
    inside = (ring >= 0) & (ring < d32.size) & ~np.isnan(d)
    out = v.copy()
    with np.errstate(over="ignore", under="ignore"):
        out[inside] = (v[inside] / d32[ring[inside]][:, None]).astype(np.float32)
    return out


# ---- the kernel --------------------------------------------------------------------------------------------------------
def _device_rows(t, name: str, cols: Optional[int], device=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: ring_scale only runs on an MI355X (no CPU fallback; ring_scale_numpy is the host-side "
                           "definition)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, dist on {device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be torch.float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if cols is None:
        if t.dim() != 1:
            raise RuntimeError(f"{name} must be [n], got {tuple(t.shape)}")
    elif t.dim() != 2 or t.shape[1] != cols:
        raise RuntimeError(f"{name} must be [n,{cols}], got {tuple(t.shape)}")
    return t


def ring_scale(dist: torch.Tensor, values: torch.Tensor, radii, divisors, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One inr_ring_scale call on the current stream: ``values`` [n,2] scaled by the ring of ``dist`` [n] into ``out``
    (default: a new tensor; ``out=values`` scales in place).  Device fp32 contiguous tensors; a bad table raises ValueError
    and a bad tensor RuntimeError before the library is called."""
    dist = _device_rows(dist, "dist", None)
    values = _device_rows(values, "values", 2, dist.device)
    r32, d32 = _table(radii, divisors)
    n = dist.numel()
    if values.shape[0] != n:
        raise RuntimeError(f"dist has {n} rows, values {values.shape[0]}")
    if n < 1:
        raise ValueError("ring_scale of no rows")
    if out is None:
        out = torch.empty_like(values)
    else:
        out = _device_rows(out, "out", 2, dist.device)
        if out.shape[0] != n:
            raise RuntimeError(f"dist has {n} rows, out {out.shape[0]}")
    FP = C.POINTER(C.c_float)
    with torch.cuda.device(dist.device):
        L.check(L.load().inr_ring_scale(dist.data_ptr(), values.data_ptr(), out.data_ptr(), n, r32.ctypes.data_as(FP),
                                        d32.ctypes.data_as(FP), int(d32.size),
                                        torch.cuda.current_stream(dist.device).cuda_stream))
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------
@dataclass
class RingTable:
    radii: np.ndarray  # [K+1] fp64, as the partition gave them (compared after rounding to fp32)
    divisors: np.ndarray  # [K] fp32
    stat: str  # "max" | "min" | "file"
    no_steps: Optional[int] = None
    no_models: Optional[int] = None

    def __post_init__(self):
        self.radii = np.asarray(self.radii, dtype=np.float64).reshape(-1)
        self.divisors = np.asarray(self.divisors, dtype=np.float32).reshape(-1)
        _table(self.radii, self.divisors)

    @property
    def rings(self) -> int:
        return int(self.divisors.size)

    @property
    def inverse(self) -> np.ndarray:
        return inverse_divisors(self.divisors)

    @classmethod
    def from_rows(cls, values: torch.Tensor, dist: torch.Tensor, no_steps: int = 40, no_models: int = 4,
                  stat: str = "max") -> "RingTable":
        """The k-means partition of the rows' log-magnitude against radius (clustering.partition_rows) and, per ring of
        it, the max (or min) of |component| (clustering.partition_and_stats_rows) -- over CLOSED ring intervals, see the
        module docstring.  ``values`` [n,2], ``dist`` [n]; device fp32 tensors take the band kernel."""
        if stat not in STATS:
            raise ValueError(f"stat {stat!r} (one of {STATS})")
        from .clustering import partition_and_stats_rows
        stats, radii = partition_and_stats_rows(values, dist, int(no_steps), int(no_models), stat)
        return cls(np.asarray(radii, dtype=np.float64), stats.detach().cpu().numpy().astype(np.float32), stat,
                   int(no_steps), int(no_models))

    @classmethod
    def from_file(cls, path: str) -> "RingTable":
        """an .npz holding ``radii`` [K+1] and ``divisors`` [K]"""
        with np.load(path) as z:
            if "radii" not in z.files or "divisors" not in z.files:
                raise ValueError(f"{path}: a ring table file holds 'radii' and 'divisors' (has {sorted(z.files)})")
            return cls(z["radii"].astype(np.float64), z["divisors"].astype(np.float32), "file")

    def summary(self) -> dict:
        """what the JSON result, metrics() and the validation records carry"""
        return {"stat": self.stat, "rings": self.rings, "radii": [float(r) for r in self.radii],
                "divisors": [float(d) for d in self.divisors]}

    def state(self) -> dict:
        """the checkpoint's 'ring_normalization' entry"""
        return {"radii": torch.from_numpy(self.radii.copy()), "divisors": torch.from_numpy(self.divisors.copy()),
                "stat": self.stat, "no_steps": self.no_steps, "no_models": self.no_models}

    @classmethod
    def from_state(cls, st: dict) -> "RingTable":
        to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return cls(to_np(st["radii"]).astype(np.float64), to_np(st["divisors"]).astype(np.float32), str(st["stat"]),
                   st.get("no_steps"), st.get("no_models"))

    def scale(self, dist: torch.Tensor, values: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """data units -> normalised units"""
        return ring_scale(dist, values, self.radii, self.divisors, out)

    def unscale(self, dist: torch.Tensor, values: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """normalised units -> data units"""
        return ring_scale(dist, values, self.radii, self.inverse, out)


def same_table(a: Optional[dict], b: Optional[dict]) -> Optional[str]:
    """None when two checkpoint entries (or absences) describe the same table -- the same fp32 radii and divisors, bit
    for bit -- else what differs"""
    if (a is None) != (b is None):
        return "one side has ring normalisation and the other has none"
    if a is None:
        return None
    ta, tb = RingTable.from_state(a), RingTable.from_state(b)
    if ta.rings != tb.rings:
        return f"ring normalisation with {ta.rings} rings against {tb.rings}"
    if not np.array_equal(ta.radii.astype(np.float32), tb.radii.astype(np.float32)):
        return "the radii of the ring normalisation differ"
    if not np.array_equal(ta.divisors, tb.divisors):
        return "the divisors of the ring normalisation differ"
    return None


# ---- config key and command line ---------------------------------------------------------------------------------------
def parse_ring_normalization(value):
    """config['ring_normalization']: None (off) | 'max' | 'min' | the path of a FILE.npz"""
    if value is None or value is False:
        return None
    text = str(value)
    if text.lower() == "none":
        return None
    if text in STATS:
        return text
    if text.lower().endswith(".npz"):
        return text
    raise ValueError(f"ring_normalization = {value!r}: none | max | min | FILE.npz")


def partition_counts(config: dict):
    """(no_steps, no_models) of config['partition'], 40 / 4 where it names none"""
    part = config.get("partition") or {}
    return int(part.get("no_steps", 40)), int(part.get("no_models", 4))


def check_ring_normalization(config: dict, mask) -> Optional[str]:
    """The parsed key, after refusing what a ring-normalised fit cannot be combined with -- before anything is allocated."""
    spec = parse_ring_normalization(config.get("ring_normalization"))
    if spec is None:
        return None
    if config.get("transform", False):
        raise ValueError(f"ring_normalization = {spec!r} with transform: true -- image space has no radial fall-off")
    from .undersampling import parse_undersampling_argument
    method = parse_undersampling_argument(config.get("undersampling"))[0]
    if (method is not None and method.lower() != "none") or mask is not None:
        raise ValueError(f"ring_normalization = {spec!r} with an undersampling pattern or a mask: a ring may hold no "
                         "sampled row (normalised fits of undersampled scans are not supported)")
    return spec


def make_table(spec: str, config: dict, values: torch.Tensor, dist: torch.Tensor) -> RingTable:
    if spec in STATS:
        return RingTable.from_rows(values, dist, *partition_counts(config), stat=spec)
    return RingTable.from_file(spec)


def add_ring_normalize_flag(ap) -> None:
    ap.add_argument("--ring-normalize", type=str, default=None, metavar="ARG",
                    help="python -m inr_mi355x.train only (the other drivers refuse it): fit ring-normalised targets: every k-means ring of k-space divided by its max | min, or by the "
                         "table of FILE.npz (radii, divisors); scores and pictures stay in the data's units "
                         "(config['ring_normalization']; none: off)")


def apply_ring_normalize_flag(config: dict, opts) -> dict:
    if getattr(opts, "ring_normalize", None) is not None:
        config["ring_normalization"] = opts.ring_normalize
    return config
