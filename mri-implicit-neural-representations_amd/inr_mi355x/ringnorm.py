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

The continuous divisor (inr_radial_scale, csrc/inr_radial_scale.hip; no reference counterpart).
``ring_profile: linear | geometric`` replaces the step function by a curve through ``divisors[r]`` at the ring centres,
constant before the first and behind the last centre, sampled on ``ring_profile_knots`` uniform knots over
``[radii[0], radii[K]]`` (``ring_profile``).  Per row, every line one correctly rounded fp32 operation::

    s  = d - r_lo
    u  = s * inv_step
    u  = u < 0 ? 0 : (u > n_knots-1 ? n_knots-1 : u)
    k  = min((int)u, n_knots - 2);   t = u - (float)k          (exact)
    df = p[k+1] - p[k];   pr = t * df;   q = p[k] + pr
    out = multiply ? in * q : in / q                           (both components)

and a row whose ``dist`` is NaN is copied bit for bit.  The inverse multiplies by the same ``q``: there is no reciprocal
table.  ``radial_scale_numpy`` is this definition in numpy, ``radial_scale_float64`` the same arithmetic in float64 and
``radial_scale`` the kernel.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _lib as L

STATS = ("max", "min")
PROFILES = ("step", "linear", "geometric")
DEFAULT_KNOTS = 1024


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
def _device_rows(t, name: str, cols: Optional[int], device=None, who: str = "ring_scale") -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: {who} only runs on an MI355X (no CPU fallback; {who}_numpy is the host-side "
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
    L.launch("inr_ring_scale", dist.device, dist.data_ptr(), values.data_ptr(), out.data_ptr(), n,
             r32.ctypes.data_as(FP), d32.ctypes.data_as(FP), int(d32.size))
    return out


# ---- the continuous divisor: profile, numpy restatement, kernel ------------------------------------------------------------
def _knots(n_knots) -> int:
    if isinstance(n_knots, bool) or int(n_knots) != n_knots or not 2 <= int(n_knots) <= L.RADIAL_KNOTS_MAX:
        raise ValueError(f"ring_profile_knots = {n_knots!r} (2..{L.RADIAL_KNOTS_MAX})")
    return int(n_knots)


def ring_profile(radii, divisors, mode: str, n_knots: int):
    """(profile fp32 [n_knots], r_lo fp32, inv_step fp32) of a ring table, built in float64.  The curve has the value
    ``divisors[r]`` at the ring centre ``c_r = (radii[r] + radii[r+1]) / 2``, is constant on ``[radii[0], c_0]`` and
    ``[c_{K-1}, radii[K]]``, and between two centres interpolates the divisor (``linear``) or its logarithm
    (``geometric``).  It is sampled at ``n_knots`` uniform radii over ``[radii[0], radii[K]]`` and rounded to fp32 once;
    ``inv_step = fl32((n_knots - 1) / (radii[K] - radii[0]))``.  One ring gives a constant profile.  Divisors must be
    positive here (a step table from a file may hold negative ones)."""
    if mode not in PROFILES[1:]:
        raise ValueError(f"ring_profile mode {mode!r} (one of {PROFILES[1:]})")
    n_knots = _knots(n_knots)
    r, d32 = _table(radii, divisors)
    R = np.asarray(radii, dtype=np.float64).reshape(-1)
    d = d32.astype(np.float64)
    K = d.size
    if np.any(d <= 0):
        raise ValueError(f"ring_profile = {mode!r} needs positive divisors (has {float(d.min())!r})")
    if not np.all(np.isfinite(R)) or not R[K] > R[0]:
        raise ValueError(f"ring_profile = {mode!r} needs finite radii with radii[0] < radii[K] (has {R[0]!r}, {R[K]!r})")
    x = R[0] + (R[K] - R[0]) * np.arange(n_knots, dtype=np.float64) / (n_knots - 1)
    if K == 1:
        curve = np.full(n_knots, d[0])
    else:
        c = 0.5 * (R[:-1] + R[1:])
        j = np.clip(np.searchsorted(c, x, side="right") - 1, 0, K - 2)
        width = c[j + 1] - c[j]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(width > 0, np.clip((x - c[j]) / width, 0.0, 1.0), 1.0)
        if mode == "linear":
            curve = d[j] + t * (d[j + 1] - d[j])
        else:
            curve = d[j] * (d[j + 1] / d[j]) ** t
        curve = np.where(t == 1.0, d[j + 1], curve)  # exactly the divisor at (and behind) a centre
    return curve.astype(np.float32), np.float32(R[0]), np.float32((n_knots - 1) / (R[K] - R[0]))


def _profile_args(profile, r_lo, inv_step, dtype):
    p = np.ascontiguousarray(profile, dtype=np.float32).reshape(-1)
    _knots(p.size)
    r_lo, inv_step = np.float32(r_lo), np.float32(inv_step)
    if not np.isfinite(r_lo):
        raise ValueError(f"r_lo = {float(r_lo)!r} (must be finite)")
    if not (np.isfinite(inv_step) and inv_step > 0):
        raise ValueError(f"inv_step = {float(inv_step)!r} (must be finite and positive)")
    return p.astype(dtype), dtype(r_lo), dtype(inv_step)


def _radial_scale_host(dist, values, profile, r_lo, inv_step, multiply, dtype) -> np.ndarray:
    """the definition in ``dtype`` arithmetic, from the fp32 inputs; every numpy operation rounds once"""
    as_np = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
    d = as_np(dist).reshape(-1).astype(dtype)
    v = as_np(values).reshape(-1, 2).astype(dtype)
    p, r_lo, inv_step = _profile_args(profile, r_lo, inv_step, dtype)
    if v.shape[0] != d.size:
        raise ValueError(f"dist has {d.size} rows, values {v.shape[0]}")
    hi = dtype(p.size - 1)
    nan = np.isnan(d)
    with np.errstate(all="ignore"):
        s = d - r_lo
        u = s * inv_step
        u = np.where(u < 0, dtype(0), np.where(u > hi, hi, u))
        u = np.where(nan, dtype(0), u)  # such a row is copied
        k = np.minimum(u.astype(np.int32), p.size - 2)
        t = u - k.astype(dtype)
        df = p[k + 1] - p[k]
        pr = t * df
        q = (p[k] + pr)[:, None]
        out = v * q if multiply else v / q
    out[nan] = v[nan]
    assert out.dtype == dtype
    return out


def radial_scale_numpy(dist, values, profile, r_lo, inv_step, multiply: bool = False) -> np.ndarray:
    """The definition of the module docstring, operation for operation in np.float32: [n,2] fp32.  Arrays or CPU tensors;
    the input is not modified."""
    return _radial_scale_host(dist, values, profile, r_lo, inv_step, multiply, np.float32)


def radial_scale_float64(dist, values, profile, r_lo, inv_step, multiply: bool = False) -> np.ndarray:
    """The same arithmetic in float64 from the same fp32 inputs: [n,2] fp64 (what radial_scale_numpy is bounded against)"""
    return _radial_scale_host(dist, values, profile, r_lo, inv_step, multiply, np.float64)


def radial_scale(dist: torch.Tensor, values: torch.Tensor, profile_dev: torch.Tensor, r_lo, inv_step,
                 multiply: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One inr_radial_scale call on the current stream: ``values`` [n,2] divided (``multiply``: multiplied) by the profile
    ``profile_dev`` (device fp32 [n_knots]) at ``dist`` [n], into ``out`` (default: a new tensor; ``out=values`` works in
    place).  Device fp32 contiguous tensors; a bad knot count, ``r_lo`` or ``inv_step`` raises ValueError and a bad tensor
    RuntimeError before the library is called."""
    who = "radial_scale"
    dist = _device_rows(dist, "dist", None, who=who)
    values = _device_rows(values, "values", 2, dist.device, who=who)
    profile_dev = _device_rows(profile_dev, "profile_dev", None, dist.device, who=who)
    n_knots = _knots(profile_dev.numel())
    r_lo, inv_step = np.float32(r_lo), np.float32(inv_step)
    if not np.isfinite(r_lo):
        raise ValueError(f"r_lo = {float(r_lo)!r} (must be finite)")
    if not (np.isfinite(inv_step) and inv_step > 0):
        raise ValueError(f"inv_step = {float(inv_step)!r} (must be finite and positive)")
    n = dist.numel()
    if values.shape[0] != n:
        raise RuntimeError(f"dist has {n} rows, values {values.shape[0]}")
    if n < 1:
        raise ValueError("radial_scale of no rows")
    if out is None:
        out = torch.empty_like(values)
    else:
        out = _device_rows(out, "out", 2, dist.device, who=who)
        if out.shape[0] != n:
            raise RuntimeError(f"dist has {n} rows, out {out.shape[0]}")
    L.launch("inr_radial_scale", dist.device, dist.data_ptr(), values.data_ptr(), out.data_ptr(), n,
             profile_dev.data_ptr(), n_knots, float(r_lo), float(inv_step), 1 if multiply else 0)
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------
@dataclass
class RingTable:
    radii: np.ndarray  # [K+1] fp64, as the partition gave them (compared after rounding to fp32)
    divisors: np.ndarray  # [K] fp32
    stat: str  # "max" | "min" | "file"
    no_steps: Optional[int] = None
    no_models: Optional[int] = None
    profile: str = "step"  # "step" | "linear" | "geometric": the divisor across ring edges
    knots: Optional[int] = None  # of a smooth profile (DEFAULT_KNOTS); None for a step table
    normalized_max: Optional[float] = field(default=None, compare=False)  # smooth tables: see note_scaled

    def __post_init__(self):
        self.radii = np.asarray(self.radii, dtype=np.float64).reshape(-1)
        self.divisors = np.asarray(self.divisors, dtype=np.float32).reshape(-1)
        _table(self.radii, self.divisors)
        if self.profile not in PROFILES:
            raise ValueError(f"ring_profile = {self.profile!r}: step | linear | geometric")
        self._curve = self._curve_dev = None
        if self.smooth:
            self.knots = _knots(DEFAULT_KNOTS if self.knots is None else self.knots)
            self._curve = ring_profile(self.radii, self.divisors, self.profile, self.knots)
            self._curve_dev = {}  # device -> the profile's copy there, made once
        else:
            self.knots = None

    @property
    def smooth(self) -> bool:
        return self.profile != "step"

    @property
    def curve(self):
        """(profile fp32 [knots], r_lo fp32, inv_step fp32) of a smooth table (ring_profile)"""
        if not self.smooth:
            raise ValueError("a step table has no profile curve")
        return self._curve

    def _radial(self, dist, values, out, multiply: bool) -> torch.Tensor:
        p, r_lo, inv_step = self._curve
        dev = self._curve_dev.get(dist.device)
        if dev is None:
            dev = self._curve_dev[dist.device] = torch.from_numpy(p.copy()).to(dist.device)
        return radial_scale(dist, values, dev, r_lo, inv_step, multiply, out)

    def note_scaled(self, scaled: torch.Tensor) -> None:
        """``scaled``: the training rows after scale().  A smooth table records their largest |component| (one torch
        reduction): unlike a step table's max-normalised rows they may exceed 1 near the inner edge of a ring."""
        if self.smooth:
            self.normalized_max = float(scaled.abs().max())

    @property
    def rings(self) -> int:
        return int(self.divisors.size)

    @property
    def inverse(self) -> np.ndarray:
        return inverse_divisors(self.divisors)

    @classmethod
    def from_rows(cls, values: torch.Tensor, dist: torch.Tensor, no_steps: int = 40, no_models: int = 4,
                  stat: str = "max", profile: str = "step", knots: Optional[int] = None) -> "RingTable":
        """The k-means partition of the rows' log-magnitude against radius (clustering.partition_rows) and, per ring of
        it, the max (or min) of |component| (clustering.partition_and_stats_rows) -- over CLOSED ring intervals, see the
        module docstring.  ``values`` [n,2], ``dist`` [n]; device fp32 tensors take the band kernel."""
        if stat not in STATS:
            raise ValueError(f"stat {stat!r} (one of {STATS})")
        from .clustering import partition_and_stats_rows
        stats, radii = partition_and_stats_rows(values, dist, int(no_steps), int(no_models), stat)
        return cls(np.asarray(radii, dtype=np.float64), stats.detach().cpu().numpy().astype(np.float32), stat,
                   int(no_steps), int(no_models), profile, knots)

    @classmethod
    def from_file(cls, path: str, profile: str = "step", knots: Optional[int] = None) -> "RingTable":
        """an .npz holding ``radii`` [K+1] and ``divisors`` [K]"""
        with np.load(path) as z:
            if "radii" not in z.files or "divisors" not in z.files:
                raise ValueError(f"{path}: a ring table file holds 'radii' and 'divisors' (has {sorted(z.files)})")
            return cls(z["radii"].astype(np.float64), z["divisors"].astype(np.float32), "file", profile=profile, knots=knots)

    def summary(self) -> dict:
        """what the JSON result, metrics() and the validation records carry; a smooth table adds its profile mode, its knot
        count and normalized_max (None where no fit scaled rows with this table: a checkpoint's)"""
        rec = {"stat": self.stat, "rings": self.rings, "radii": [float(r) for r in self.radii],
               "divisors": [float(d) for d in self.divisors]}
        if self.smooth:
            rec.update(profile=self.profile, knots=self.knots, normalized_max=self.normalized_max)
        return rec

    def state(self) -> dict:
        """the checkpoint's 'ring_normalization' entry; a smooth table adds its profile mode and knot count"""
        st = {"radii": torch.from_numpy(self.radii.copy()), "divisors": torch.from_numpy(self.divisors.copy()),
              "stat": self.stat, "no_steps": self.no_steps, "no_models": self.no_models}
        if self.smooth:
            st.update(profile=self.profile, knots=self.knots)
        return st

    @classmethod
    def from_state(cls, st: dict) -> "RingTable":
        to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return cls(to_np(st["radii"]).astype(np.float64), to_np(st["divisors"]).astype(np.float32), str(st["stat"]),
                   st.get("no_steps"), st.get("no_models"), str(st.get("profile", "step")), st.get("knots"))

    def scale(self, dist: torch.Tensor, values: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """data units -> normalised units"""
        if self.smooth:
            return self._radial(dist, values, out, multiply=False)
        return ring_scale(dist, values, self.radii, self.divisors, out)

    def unscale(self, dist: torch.Tensor, values: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """normalised units -> data units (a smooth table multiplies by the same profile: no reciprocal table)"""
        if self.smooth:
            return self._radial(dist, values, out, multiply=True)
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
    if ta.profile != tb.profile:
        return f"ring normalisation with profile {ta.profile!r} against {tb.profile!r}"
    if ta.knots != tb.knots:
        return f"ring normalisation with {ta.knots} profile knots against {tb.knots}"
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


def parse_ring_profile(value) -> str:
    """config['ring_profile']: 'step' (the default: one divisor per ring) | 'linear' | 'geometric'"""
    if value is None:
        return "step"
    if isinstance(value, str) and value in PROFILES:
        return value
    raise ValueError(f"ring_profile = {value!r}: step | linear | geometric")


def check_ring_profile(config: dict, spec: Optional[str]):
    """(profile, knots) of config['ring_profile'] / ['ring_profile_knots'] beside the parsed ring_normalization ``spec``;
    knots is None for a step profile"""
    profile = parse_ring_profile(config.get("ring_profile"))
    if profile == "step":
        return profile, None
    if spec is None:
        raise ValueError(f"ring_profile = {profile!r} without ring_normalization: there is no ring table to smooth")
    knots = config.get("ring_profile_knots")
    return profile, _knots(DEFAULT_KNOTS if knots is None else knots)


def check_ring_normalization(config: dict, mask) -> Optional[str]:
    """The parsed key, after refusing what a ring-normalised fit cannot be combined with -- before anything is allocated."""
    spec = parse_ring_normalization(config.get("ring_normalization"))
    check_ring_profile(config, spec)
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
    profile, knots = check_ring_profile(config, spec)
    if spec in STATS:
        return RingTable.from_rows(values, dist, *partition_counts(config), stat=spec, profile=profile, knots=knots)
    return RingTable.from_file(spec, profile=profile, knots=knots)


def add_ring_normalize_flag(ap) -> None:
    ap.add_argument("--ring-profile", type=str, default=None, metavar="ARG",
                    help="with --ring-normalize: the divisor across ring edges: step (one constant per ring) | linear | "
                         "geometric (a continuous curve through the divisors at the ring centres, interpolating the divisor "
                         "or its logarithm) (config['ring_profile']; default step)")
    ap.add_argument("--ring-profile-knots", type=int, default=None, metavar="N",
                    help="uniform knots the continuous profile is sampled on, 2..4096 (config['ring_profile_knots']; "
                         "default 1024)")
    ap.add_argument("--ring-normalize", type=str, default=None, metavar="ARG",
                    help="python -m inr_mi355x.train only (the other drivers refuse it): fit ring-normalised targets: every k-means ring of k-space divided by its max | min, or by the "
                         "table of FILE.npz (radii, divisors); scores and pictures stay in the data's units "
                         "(config['ring_normalization']; none: off)")


def apply_ring_normalize_flag(config: dict, opts) -> dict:
    if getattr(opts, "ring_normalize", None) is not None:
        config["ring_normalization"] = opts.ring_normalize
    if getattr(opts, "ring_profile", None) is not None:
        config["ring_profile"] = opts.ring_profile
    if getattr(opts, "ring_profile_knots", None) is not None:
        config["ring_profile_knots"] = opts.ring_profile_knots
    return config
