"""Off-grid fits (inr_nudft, csrc/inr_nudft.hip): train a coordinate network on k-space samples that do
not lie on the Cartesian grid -- radial spokes, or any measured trajectory -- with no gridding step.  The reference has no
counterpart; the switch is config['trajectory'] (absent or "none": off, and then nothing here runs).

A Cartesian scan is sampled retrospectively.  For a coil image I[y][x] (complex, H x W, centred as evalchain.ifft2c leaves
it) the continuous k-space at the fractional index position (u_y, u_x) is

    K(u_y, u_x) = 1/sqrt(H W) sum_y sum_x I[y][x] exp(-2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)),
    c_y = H // 2, c_x = W // 2

which at integer positions is evalchain.fft2c(I)[u_y][u_x] for every parity of H and W.  The network coordinate of a
position is -1 + 2 u / (n - 1) per axis, formed in fp64 and rounded to fp32 (grid points keep their create_coords values to
one ulp); the coil coordinate is linspace(-1, 1, C)[c], as on the grid.

``nudft_numpy`` is the definition in fp64 and needs no GPU; ``nudft`` is the device call, which reduces the phase in fp64
and forms phasors and sums in fp32.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L

GOLDEN_ANGLE = math.pi * (math.sqrt(5.0) - 1.0) / 2.0  # radians between consecutive spokes


# ---- trajectories ------------------------------------------------------------------------------------------------------
def spokes(H: int, W: int, n_spokes: int, readout: Optional[int] = None, first: int = 0) -> np.ndarray:
    """fp64 [n_spokes * R, 2] positions (u_y, u_x), spoke-major.  Spoke s has angle (first + s) * GOLDEN_ANGLE; sample j of
    R = readout or max(H, W) has rho_j = (j - R // 2) / (R // 2); u = c + rho_j * a * (sin, cos) with c = n // 2 and
    a = min(c, n - 1 - c) per axis, so every sample stays inside the grid and sample R // 2 is the centre."""
    H, W, n_spokes, first = int(H), int(W), int(n_spokes), int(first)
    R = int(readout) if readout else max(H, W)
    if H < 1 or W < 1 or n_spokes < 1 or R < 2:
        raise ValueError(f"spokes: H = {H}, W = {W}, n_spokes = {n_spokes}, readout = {R} (H, W, n_spokes >= 1, readout >= 2)")
    cy, cx = H // 2, W // 2
    ay, ax = min(cy, H - 1 - cy), min(cx, W - 1 - cx)
    theta = (first + np.arange(n_spokes, dtype=np.float64)) * GOLDEN_ANGLE
    rho = (np.arange(R, dtype=np.float64) - R // 2) / (R // 2)
    pos = np.empty((n_spokes, R, 2), dtype=np.float64)
    pos[:, :, 0] = cy + rho[None, :] * (ay * np.sin(theta))[:, None]
    pos[:, :, 1] = cx + rho[None, :] * (ax * np.cos(theta))[:, None]
    # rho runs to (R - 1 - R // 2) / (R // 2) <= 1 and |sin|, |cos| <= 1: inside [c - a, c + a], a subset of [0, n - 1]
    return pos.reshape(-1, 2)


def parse_trajectory(arg):
    """config['trajectory'] -> None (off), ("spokes", N, R or None) or ("file", path, positions [M, 2] fp64).  Accepts
    None / "none", "spokes-N", "spokes-N-R" and the path of a .npy file of [M, 2] float64 positions, which must be
    finite.  ValueError for anything else."""
    if arg is None:
        return None
    if not isinstance(arg, str):
        raise ValueError(f"trajectory = {arg!r}: 'none', 'spokes-N', 'spokes-N-R' or the path of a .npy file")
    if arg.lower() == "none":
        return None
    m = re.fullmatch(r"spokes-(\d+)(?:-(\d+))?", arg)
    if m:
        n, r = int(m.group(1)), (int(m.group(2)) if m.group(2) else None)
        if n < 1 or (r is not None and r < 2):
            raise ValueError(f"trajectory = {arg!r}: at least one spoke of at least two samples")
        return ("spokes", n, r)
    if arg.endswith(".npy"):
        if not os.path.isfile(arg):
            raise ValueError(f"trajectory = {arg!r}: no such file")
        pos = np.load(arg, allow_pickle=False)
        return ("file", arg, check_positions(pos, arg))
    raise ValueError(f"trajectory = {arg!r}: 'none', 'spokes-N', 'spokes-N-R' or the path of a .npy file")


def check_positions(pos, what: str = "positions") -> np.ndarray:
    """[M, 2] finite float64 positions, contiguous; ValueError otherwise"""
    pos = np.asarray(pos)
    if pos.ndim != 2 or pos.shape[1] != 2 or pos.shape[0] < 1 or pos.dtype != np.float64:
        raise ValueError(f"{what}: expected [M, 2] float64 positions (u_y, u_x), got {pos.dtype} {pos.shape}")
    if not np.isfinite(pos).all():
        raise ValueError(f"{what}: non-finite position")
    return np.ascontiguousarray(pos)


def positions(parsed, H: int, W: int) -> np.ndarray:
    """the [M, 2] fp64 positions of a parsed trajectory on an H x W grid"""
    if parsed[0] == "spokes":
        return spokes(H, W, parsed[1], parsed[2])
    return parsed[2]


def describe(parsed, H: int, W: int) -> Optional[dict]:
    """what the JSON result and the validation records carry: {kind, spokes, readout, rows_per_coil, acceleration}"""
    if parsed is None:
        return None
    if parsed[0] == "spokes":
        R = parsed[2] or max(int(H), int(W))
        n, M = parsed[1], parsed[1] * R
        return {"kind": "spokes", "spokes": n, "readout": R, "rows_per_coil": M, "acceleration": H * W / M}
    M = int(parsed[2].shape[0])
    return {"kind": "file", "spokes": None, "readout": None, "rows_per_coil": M, "acceleration": H * W / M}


def trajectory_coords(pos, C_: int, H: int, W: int) -> torch.Tensor:
    """fp32 [C * M, 3] rows (coil, y, x), coil-major: -1 + 2 u / (n - 1) in fp64 (-1 on an axis of one point, the value
    linspace(-1, 1, 1) gives the grid), rounded to fp32"""
    pos = check_positions(pos)
    M = pos.shape[0]

    def axis(u, n):
        return np.full_like(u, -1.0) if n == 1 else -1.0 + 2.0 * u / (n - 1)

    z = np.linspace(-1.0, 1.0, int(C_)) if C_ > 1 else np.array([-1.0])
    rows = np.empty((int(C_), M, 3), dtype=np.float32)
    rows[:, :, 0] = z.astype(np.float32)[:, None]
    rows[:, :, 1] = axis(pos[:, 0], int(H)).astype(np.float32)[None, :]
    rows[:, :, 2] = axis(pos[:, 1], int(W)).astype(np.float32)[None, :]
    return torch.from_numpy(rows.reshape(-1, 3))


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def _phasors(u: np.ndarray, n: int) -> np.ndarray:
    """[M, n] complex128: exp(-2 pi i frac((u - c)(j - c) / n))"""
    c = n // 2
    t = (u[:, None] - c) * (np.arange(n, dtype=np.float64) - c)[None, :] / n
    t = t - np.rint(t)
    return np.exp(-2j * np.pi * t)


def nudft_numpy(img, pos) -> np.ndarray:
    """[C, M] complex128.  ``img``: [C, H, W, 2] pairs (array or CPU tensor) or a complex [C, H, W] array; ``pos``: [M, 2]."""
    from .coils import _as_complex
    z = np.asarray(_as_complex(img)).astype(np.complex128)
    if z.ndim == 2:
        z = z[None]
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    Cn, H, W = z.shape
    ey, ex = _phasors(pos[:, 0], H), _phasors(pos[:, 1], W)
    out = np.empty((Cn, pos.shape[0]), dtype=np.complex128)
    for c in range(Cn):
        out[c] = ((ex @ z[c].T) * ey).sum(axis=1)  # T[m][y] = sum_x Ex[m][x] I[y][x], then sum_y Ey[m][y] T[m][y]
    return out / math.sqrt(H * W)


def error_bound(img, H: int, W: int) -> np.ndarray:
    """[C] fp64: (H W + 32) 2^-24 sum |I_c| / sqrt(H W) -- the worst-case fp32 bound of |nudft - nudft_numpy| per output:
    H W accumulated terms, each formed with a few roundings after an fp64-reduced phase"""
    from .coils import _as_complex
    z = np.asarray(_as_complex(img)).astype(np.complex128)
    if z.ndim == 2:
        z = z[None]
    return (H * W + 32) * 2.0 ** -24 * np.abs(z).reshape(z.shape[0], -1).sum(axis=1) / math.sqrt(H * W)


# ---- the kernel --------------------------------------------------------------------------------------------------------
def scratch_floats(coils: int, H: int, W: int, M: int) -> int:
    out = C.c_int64(0)
    L.check(L.load().inr_nudft_scratch(int(coils), int(H), int(W), int(M), C.byref(out)))
    return int(out.value)


def nudft(img: torch.Tensor, pos, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[C, M, 2] fp32 on the device: K_c(pos[m]) of the coil images ``img`` [C, H, W, 2] (device, fp32).  ``pos``: [M, 2]
    fp64, a numpy array or a device tensor.  One inr_nudft call on the current stream; ``scratch``: a float32 device
    buffer of at least scratch_floats(C, H, W, M) entries (default: allocated here)."""
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise RuntimeError("nudft only runs on an MI355X (no CPU fallback; nudft_numpy is the host-side definition)")
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[-1] != 2:
        raise RuntimeError(f"img must be float32 [C, H, W, 2] (got {img.dtype} {tuple(img.shape)})")
    img = img.contiguous()
    coils, H, W = (int(v) for v in img.shape[:3])
    if isinstance(pos, torch.Tensor):
        if pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 2:
            raise ValueError(f"pos: expected [M, 2] float64, got {pos.dtype} {tuple(pos.shape)}")
        p = pos.to(img.device).contiguous()
    else:
        p = torch.from_numpy(check_positions(pos)).to(img.device)
    M = int(p.shape[0])
    need = scratch_floats(coils, H, W, M)
    if scratch is None:
        scratch = torch.empty(need, device=img.device, dtype=torch.float32)
    out = torch.empty(coils, M, 2, device=img.device, dtype=torch.float32)
    with torch.cuda.device(img.device):
        L.check(L.load().inr_nudft(img.data_ptr(), coils, H, W, p.data_ptr(), M, out.data_ptr(), scratch.data_ptr(),
                                   scratch.numel(), torch.cuda.current_stream(img.device).cuda_stream))
    return out


def sample_kspace(kspace: torch.Tensor, shape, pos) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values [(C*M), 2] on the device, coords [(C*M), 3] fp32 on the host) of the off-grid rows of a resident k-space
    [(C*H*W), 2]: ifft2c, then nudft"""
    from .evalchain import ifft2c
    C_, H, W = (int(v) for v in shape[:3])
    img = ifft2c(kspace.reshape(C_, H, W, 2)).contiguous()
    return nudft(img, pos).reshape(-1, 2), trajectory_coords(pos, C_, H, W)


# ---- the switch --------------------------------------------------------------------------------------------------------
def add_trajectory_flag(ap) -> None:
    ap.add_argument("--trajectory", type=str, default=None, metavar="ARG",
                    help="train on off-grid k-space samples: spokes-N, spokes-N-R (golden-angle spokes of R samples) or a "
                         ".npy file of [M,2] float64 index positions (config['trajectory']; none: off)")


def apply_trajectory_flag(config: dict, opts) -> dict:
    if getattr(opts, "trajectory", None) is not None:
        config["trajectory"] = opts.trajectory
    return config
