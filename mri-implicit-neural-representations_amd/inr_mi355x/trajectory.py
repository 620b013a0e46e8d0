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

``nudft_adjoint`` (inr_adjoint_nudft, csrc/inr_nudft_adjoint.hip) is the conjugate transpose, with optional
density weights; ``cg_baseline`` builds the conventional density-weighted conjugate-gradient reconstruction from the two,
which config['trajectory_baseline'] prints next to the fit's score.

``nufft`` / ``nufft_adjoint`` (inr_nufft_*, csrc/inr_nufft.hip) approximate the same two operators by
Kaiser-Bessel gridding around torch.fft; config['trajectory_operator'] = "gridding" puts them inside the baseline.
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


def _image_complex(img) -> np.ndarray:
    """[C, H, W] complex128 of [C, H, W, 2] pairs (array or CPU tensor) or a complex [C, H, W] / [H, W] array"""
    from .coils import _as_complex
    z = np.asarray(_as_complex(img)).astype(np.complex128)
    return z[None] if z.ndim == 2 else z


def nudft_numpy(img, pos) -> np.ndarray:
    """[C, M] complex128.  ``img``: [C, H, W, 2] pairs (array or CPU tensor) or a complex [C, H, W] array; ``pos``: [M, 2]."""
    z = _image_complex(img)
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
    z = _image_complex(img)
    return (H * W + 32) * 2.0 ** -24 * np.abs(z).reshape(z.shape[0], -1).sum(axis=1) / math.sqrt(H * W)


# ---- the kernel --------------------------------------------------------------------------------------------------------
def _scratch_query(entry: str, coils: int, H: int, W: int, M: int) -> int:
    out = C.c_int64(0)
    L.check(getattr(L.load(), entry)(int(coils), int(H), int(W), int(M), C.byref(out)))
    return int(out.value)


def _device_pairs(t, who: str, name: str, dims: str, host: str) -> torch.Tensor:
    """the contiguous float32 device tensor ``name`` of (re, im) pairs, ``dims`` naming its leading axes"""
    rank = dims.count(",") + 2
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who} only runs on an MI355X (no CPU fallback; {host})")
    if t.dtype != torch.float32 or t.dim() != rank or t.shape[-1] != 2:
        raise RuntimeError(f"{name} must be float32 [{dims}, 2] (got {t.dtype} {tuple(t.shape)})")
    return t.contiguous()


def _device_positions(pos, device) -> torch.Tensor:
    if isinstance(pos, torch.Tensor):
        if pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 2:
            raise ValueError(f"pos: expected [M, 2] float64, got {pos.dtype} {tuple(pos.shape)}")
        return pos.to(device).contiguous()
    return torch.from_numpy(check_positions(pos)).to(device)


def scratch_floats(coils: int, H: int, W: int, M: int) -> int:
    return _scratch_query("inr_nudft_scratch", coils, H, W, M)


def nudft(img: torch.Tensor, pos, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[C, M, 2] fp32 on the device: K_c(pos[m]) of the coil images ``img`` [C, H, W, 2] (device, fp32).  ``pos``: [M, 2]
    fp64, a numpy array or a device tensor.  One inr_nudft call on the current stream; ``scratch``: a float32 device
    buffer of at least scratch_floats(C, H, W, M) entries (default: allocated here)."""
    img = _device_pairs(img, "nudft", "img", "C, H, W", "nudft_numpy is the host-side definition")
    coils, H, W = (int(v) for v in img.shape[:3])
    p = _device_positions(pos, img.device)
    M = int(p.shape[0])
    if scratch is None:
        scratch = torch.empty(scratch_floats(coils, H, W, M), device=img.device, dtype=torch.float32)
    out = torch.empty(coils, M, 2, device=img.device, dtype=torch.float32)
    L.launch("inr_nudft", img.device, img.data_ptr(), coils, H, W, p.data_ptr(), M, out.data_ptr(), scratch.data_ptr(),
             scratch.numel())
    return out


def sample_kspace(kspace: torch.Tensor, shape, pos) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values [(C*M), 2] on the device, coords [(C*M), 3] fp32 on the host) of the off-grid rows of a resident k-space
    [(C*H*W), 2]: ifft2c, then nudft"""
    from .evalchain import ifft2c
    C_, H, W = (int(v) for v in shape[:3])
    img = ifft2c(kspace.reshape(C_, H, W, 2)).contiguous()
    return nudft(img, pos).reshape(-1, 2), trajectory_coords(pos, C_, H, W)


# ---- the adjoint: samples back onto the grid (inr_adjoint_nudft, csrc/inr_nudft_adjoint.hip) ----------
def _samples_complex(val) -> np.ndarray:
    """[C, M] complex128 of [C, M, 2] pairs (array or CPU tensor) or a complex [C, M] / [M] array"""
    if isinstance(val, torch.Tensor):
        val = val.detach().cpu().numpy()
    v = np.asarray(val)
    if not np.iscomplexobj(v):
        if v.ndim < 2 or v.shape[-1] != 2:
            raise ValueError(f"samples: expected [C, M, 2] pairs or a complex [C, M] array, got {v.dtype} {v.shape}")
        v = v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)
    v = v.astype(np.complex128)
    return v[None] if v.ndim == 1 else v


def _weights_numpy(weights, M: int) -> np.ndarray:
    if weights is None:
        return np.ones(M, dtype=np.float64)
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (M,):
        raise ValueError(f"weights: expected [{M}], got {w.shape}")
    return w


def nudft_adjoint_numpy(val, pos, H: int, W: int, weights=None) -> np.ndarray:
    """[C, H, W] complex128: the conjugate transpose of nudft_numpy applied to weights * val,
    out[c][y][x] = 1/sqrt(H W) sum_m w[m] val[c][m] exp(+2 pi i ((u_y - c_y)(y - c_y)/H + (u_x - c_x)(x - c_x)/W)).
    ``val``: [C, M, 2] pairs or complex [C, M]; ``pos``: [M, 2]; ``weights``: [M] or None (all ones)."""
    v = _samples_complex(val)
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    H, W = int(H), int(W)
    if v.shape[1] != pos.shape[0]:
        raise ValueError(f"samples {v.shape} and positions {pos.shape} disagree")
    v = v * _weights_numpy(weights, pos.shape[0])[None, :]
    ey, ex = np.conj(_phasors(pos[:, 0], H)), np.conj(_phasors(pos[:, 1], W))  # [M, H], [M, W]
    out = np.empty((v.shape[0], H, W), dtype=np.complex128)
    for c in range(v.shape[0]):
        out[c] = (ey * v[c][:, None]).T @ ex  # sum_m conj(Ey[m][y]) v[m] conj(Ex[m][x])
    return out / math.sqrt(H * W)


def adjoint_error_bound(val, weights, H: int, W: int) -> np.ndarray:
    """[C] fp64: (M + 32) 2^-24 sum_m |w_m val_c[m]| / sqrt(H W) -- the worst-case fp32 bound of
    |nudft_adjoint - nudft_adjoint_numpy| per pixel: M accumulated terms, each formed with a few roundings after an
    fp64-reduced phase (the form of error_bound)"""
    v = _samples_complex(val)
    M = v.shape[1]
    return (M + 32) * 2.0 ** -24 * (np.abs(v) * np.abs(_weights_numpy(weights, M))[None, :]).sum(axis=1) / math.sqrt(H * W)


def adjoint_scratch_floats(coils: int, H: int, W: int, M: int) -> int:
    return _scratch_query("inr_adjoint_nudft_scratch", coils, H, W, M)


def _device_weights(weights, M: int, device) -> Optional[torch.Tensor]:
    if weights is None:
        return None
    w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.asarray(weights, dtype=np.float64))
    if tuple(w.shape) != (M,):
        raise ValueError(f"weights: expected [{M}], got {tuple(w.shape)}")
    return w.to(device=device, dtype=torch.float32).contiguous()


def nudft_adjoint(val: torch.Tensor, pos, shape, weights=None, scratch: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[C, H, W, 2] fp32 on the device: the samples ``val`` [C, M, 2] (device, fp32) at ``pos`` [M, 2] (fp64, numpy or
    device tensor), times ``weights`` [M] (any float array or tensor, used in fp32; None: ones), back on the H x W grid of
    ``shape`` = (H, W) or (C, H, W).  One inr_adjoint_nudft call on the current stream; ``scratch``: a float32 device
    buffer of at least adjoint_scratch_floats(C, H, W, M) entries (default: allocated here)."""
    val = _device_pairs(val, "nudft_adjoint", "val", "C, M", "nudft_adjoint_numpy is the host-side definition")
    coils, M = int(val.shape[0]), int(val.shape[1])
    H, W = (int(v) for v in tuple(shape)[-2:])
    p = _device_positions(pos, val.device)
    if int(p.shape[0]) != M:
        raise ValueError(f"val has {M} samples per coil, pos {int(p.shape[0])}")
    w = _device_weights(weights, M, val.device)
    if scratch is None:
        scratch = torch.empty(adjoint_scratch_floats(coils, H, W, M), device=val.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(coils, H, W, 2, device=val.device, dtype=torch.float32)
    L.launch("inr_adjoint_nudft", val.device, val.data_ptr(), p.data_ptr(), None if w is None else w.data_ptr(), coils,
             H, W, M, out.data_ptr(), scratch.data_ptr(), scratch.numel())
    return out


# ---- the same operators by Kaiser-Bessel gridding (inr_nufft_*, csrc/inr_nufft.hip) -------------------
# Fixed: oversampling 2 (G = 2 n per axis), NUFFT_TAPS = 6 taps per axis, kb(t) = I0(beta sqrt(1 - (2t/J)^2)) / I0(beta)
# on |t| <= J/2 with Beatty's beta.  A sample at u sits at g = 2 (u - c) + G/2 (fp64, reduced into [0, G)); its taps are
# the cells j0 .. j0 + 5, j0 = ceil(g - 3), modulo G, with weights kb(g - j) rounded to fp32.
#   forward:  img * 2 / (a_y a_x), centred in the zero Gy x Gx grid -> centred orthonormal FFT -> 36 taps per sample
#   adjoint:  w * val spread onto the grid by the same taps -> centred orthonormal inverse FFT -> centre H x W times
#             2 / (a_y a_x)
# with a(nu) the continuous Fourier transform of kb at nu = (y - c) / G and 2 = sqrt(Gy Gx) / sqrt(H W).
NUFFT_TAPS = 6   # INR_NUFFT_TAPS
NUFFT_TILE = 16  # INR_NUFFT_TILE: grid cells per edge of a spread tile and of a bin
NUFFT_BETA = math.pi * math.sqrt((NUFFT_TAPS / 2.0) ** 2 * 1.5 ** 2 - 0.8)
_I0_TERMS = 40  # of the power series: the first neglected term is below 1e-19 of the sum at beta


def _i0(x: np.ndarray) -> np.ndarray:
    """I0 by its power series sum_k (x^2/4)^k / (k!)^2, the text of the kernel's bessel_i0 (0 <= x <= NUFFT_BETA)"""
    q = 0.25 * np.asarray(x, dtype=np.float64) ** 2
    term, total = np.ones_like(q), np.ones_like(q)
    for k in range(1, _I0_TERMS + 1):
        term = term * (q * (1.0 / (float(k) * float(k))))
        total = total + term
    return total


def nufft_kernel(t) -> np.ndarray:
    """kb(t) in fp64; zero outside |t| <= J/2"""
    t = np.asarray(t, dtype=np.float64) * (2.0 / NUFFT_TAPS)
    r = np.maximum(0.0, 1.0 - t * t)
    return np.where(np.abs(t) <= 1.0, _i0(NUFFT_BETA * np.sqrt(r)) * (1.0 / _i0(np.float64(NUFFT_BETA))), 0.0)


def nufft_apodisation(n: int) -> np.ndarray:
    """fp32 [n]: a((y - c) / G) = J sinh(s) / (s I0(beta)), s = sqrt(beta^2 - (pi J nu)^2), evaluated in fp64.  |nu| <= 1/4,
    so s is real (pi J / 4 < beta)."""
    n = int(n)
    nu = (np.arange(n, dtype=np.float64) - n // 2) / (2.0 * n)
    s = np.sqrt(NUFFT_BETA ** 2 - (math.pi * NUFFT_TAPS * nu) ** 2)
    return (NUFFT_TAPS * np.sinh(s) / (s * _i0(np.float64(NUFFT_BETA)))).astype(np.float32)


def _nufft_grid_position(u: np.ndarray, n: int) -> np.ndarray:
    """g in [0, G), the operations of the kernel's axis_taps in the same order"""
    G = 2.0 * n
    g = 2.0 * (u - float(n // 2)) + float(n)
    g = g - G * np.floor(g / G)
    g = np.where(g >= G, g - G, g)
    return np.where((g >= 0.0) & (g < G), g, 0.0)


def nufft_taps(u, n: int):
    """(j0 int64 [M], weights fp32 [M, 6]) of the positions ``u`` [M] along an axis of n points"""
    g = _nufft_grid_position(np.asarray(u, dtype=np.float64), int(n))
    first = np.ceil(g - 0.5 * NUFFT_TAPS)
    t = g[:, None] - (first[:, None] + np.arange(NUFFT_TAPS, dtype=np.float64)[None, :])
    return first.astype(np.int64), nufft_kernel(t).astype(np.float32)


def _nufft_check_shape(H: int, W: int) -> None:
    if H < NUFFT_TAPS // 2 or W < NUFFT_TAPS // 2:
        raise ValueError(f"nufft: H = {H}, W = {W} (each >= {NUFFT_TAPS // 2}: six taps must land on six cells of 2 n)")


def _nufft_cells(pos, H: int, W: int):
    """(iy [M, 6], ix [M, 6] wrapped cell indices, wy, wx [M, 6] fp64 copies of the fp32 weights)"""
    jy, wy = nufft_taps(pos[:, 0], H)
    jx, wx = nufft_taps(pos[:, 1], W)
    k = np.arange(NUFFT_TAPS)[None, :]
    return (jy[:, None] + k) % (2 * H), (jx[:, None] + k) % (2 * W), wy.astype(np.float64), wx.astype(np.float64)


def _deapodisation(H: int, W: int) -> np.ndarray:
    """[H, W] fp64: 2 / (a_y a_x) of the fp32-stored apodisation vectors"""
    return 2.0 / (nufft_apodisation(H).astype(np.float64)[:, None] * nufft_apodisation(W).astype(np.float64)[None, :])


def _fftc_numpy(z: np.ndarray, inverse: bool) -> np.ndarray:
    z = np.fft.ifftshift(z, axes=(-2, -1))
    z = (np.fft.ifft2 if inverse else np.fft.fft2)(z, axes=(-2, -1), norm="ortho")
    return np.fft.fftshift(z, axes=(-2, -1))


def nufft_numpy(img, pos) -> np.ndarray:
    """[C, M] complex128: the gridding approximation of nudft_numpy, every step in fp64 (the tap weights and the
    apodisation vectors are the fp32 numbers the device uses)"""
    z = _image_complex(img)
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    Cn, H, W = z.shape
    _nufft_check_shape(H, W)
    grid = np.zeros((Cn, 2 * H, 2 * W), dtype=np.complex128)
    y0, x0 = H - H // 2, W - W // 2
    grid[:, y0:y0 + H, x0:x0 + W] = z * _deapodisation(H, W)[None]
    grid = _fftc_numpy(grid, False)
    iy, ix, wy, wx = _nufft_cells(pos, H, W)
    cells = grid[:, iy[:, :, None], ix[:, None, :]]  # [C, M, 6, 6]
    return np.einsum("cmyx,my,mx->cm", cells, wy, wx)


def nufft_adjoint_numpy(val, pos, H: int, W: int, weights=None) -> np.ndarray:
    """[C, H, W] complex128: the gridding approximation of nudft_adjoint_numpy and the exact conjugate transpose of
    nufft_numpy applied to weights * val"""
    v = _samples_complex(val)
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    H, W = int(H), int(W)
    _nufft_check_shape(H, W)
    if v.shape[1] != pos.shape[0]:
        raise ValueError(f"samples {v.shape} and positions {pos.shape} disagree")
    v = v * _weights_numpy(weights, pos.shape[0])[None, :]
    iy, ix, wy, wx = _nufft_cells(pos, H, W)
    grid = np.zeros((v.shape[0], 2 * H, 2 * W), dtype=np.complex128)
    contrib = v[:, :, None, None] * (wy[:, :, None] * wx[:, None, :])[None]  # [C, M, 6, 6]
    for c in range(v.shape[0]):
        np.add.at(grid[c], (np.broadcast_to(iy[:, :, None], contrib.shape[1:]),
                            np.broadcast_to(ix[:, None, :], contrib.shape[1:])), contrib[c])
    grid = _fftc_numpy(grid, True)
    y0, x0 = H - H // 2, W - W // 2
    return grid[:, y0:y0 + H, x0:x0 + W] * _deapodisation(H, W)[None]


def nufft_tile_bins(tile: int, G: int) -> list:
    """The reach rule of inr_nufft_spread along one axis: the bins, ascending, that a tile of cells
    [16 tile, min(16 tile + 15, G - 1)] walks.  A sample is binned by the cell floor(g); its taps lie in
    floor(g) - 3 .. floor(g) + 3 (j0 = ceil(g - 3) is floor(g) - 2, or floor(g) - 3 at an integer g), so the tile needs
    every bin that holds a cell of [lo - 3, hi + 3] modulo G: at most four, a narrow last bin included."""
    lo = tile * NUFFT_TILE - NUFFT_TAPS // 2
    hi = min(tile * NUFFT_TILE + NUFFT_TILE - 1, G - 1) + NUFFT_TAPS // 2
    return sorted({(cell % G) // NUFFT_TILE for cell in range(lo, hi + 1)})


def nufft_bins(pos, H: int, W: int):
    """The cell list inr_nufft_spread gathers from: (bin_start int32 [T + 1], order int32 [M]).  The 2H x 2W grid is cut
    into bins of NUFFT_TILE x NUFFT_TILE cells (the last of an axis may be narrower), T = ceil(2H / 16) ceil(2W / 16), row
    major; sample m belongs to bin (floor(g_y) // 16) * ceil(2W / 16) + floor(g_x) // 16 with g the grid position
    nufft_taps uses.  ``order`` is the stable argsort of the bin numbers, so a bin lists its samples in ascending index;
    bin b is order[bin_start[b] : bin_start[b + 1]].  Which bins a tile reads: nufft_tile_bins."""
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    H, W = int(H), int(W)
    _nufft_check_shape(H, W)
    nby, nbx = -(-2 * H // NUFFT_TILE), -(-2 * W // NUFFT_TILE)
    by = np.floor(_nufft_grid_position(pos[:, 0], H)).astype(np.int64) // NUFFT_TILE
    bx = np.floor(_nufft_grid_position(pos[:, 1], W)).astype(np.int64) // NUFFT_TILE
    b = by * nbx + bx
    order = np.argsort(b, kind="stable").astype(np.int32)
    bin_start = np.zeros(nby * nbx + 1, dtype=np.int64)
    np.cumsum(np.bincount(b, minlength=nby * nbx), out=bin_start[1:])
    return bin_start.astype(np.int32), order


def _nufft_tap_sum(pos, H: int, W: int) -> float:
    """max over the samples of (sum of the six y weights) (sum of the six x weights)"""
    _, wy = nufft_taps(pos[:, 0], H)
    _, wx = nufft_taps(pos[:, 1], W)
    return float((wy.astype(np.float64).sum(axis=1) * wx.astype(np.float64).sum(axis=1)).max())


def _gamma(n: int) -> float:
    """n roundings of fp32, compounded: n u / (1 - n u), u = 2^-24"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def _fft_roundings(H: int, W: int) -> int:
    """4 per radix-2 stage (twiddle, two in a component of the complex product, the sum) over
    ceil(log2 Gy) + ceil(log2 Gx) stages"""
    return 4 * (math.ceil(math.log2(2 * H)) + math.ceil(math.log2(2 * W)))


def nufft_error_bound(img, pos) -> np.ndarray:
    """[C] fp64: the worst-case fp32 bound of |nufft - nufft_numpy| per output,
        gamma(J^2 + 2 + 4 + 3 + 4 L) S B_c,   B_c = sum_yx |I_c| 2 / (a_y a_x) / sqrt(Gy Gx),   S = max_m (sum wy)(sum wx):
    every grid value is at most B_c; it carries 3 roundings of the apodisation and 4 per FFT stage (L stages); a sample adds
    J^2 products, each with a rounded weight product and a rounded multiplication, and the two stored weights may differ
    from the restatement's by one fp32 unit each (2 roundings each)."""
    z = _image_complex(img)
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    Cn, H, W = z.shape
    B = (np.abs(z) * _deapodisation(H, W)[None]).reshape(Cn, -1).sum(axis=1) / math.sqrt(4.0 * H * W)
    return _gamma(NUFFT_TAPS ** 2 + 2 + 4 + 3 + _fft_roundings(H, W)) * _nufft_tap_sum(pos, H, W) * B


def nufft_adjoint_error_bound(val, pos, weights, H: int, W: int) -> np.ndarray:
    """[C] fp64: the worst-case fp32 bound of |nufft_adjoint - nufft_adjoint_numpy| per pixel,
        gamma(M + 2 + 4 + 3 + 4 L) D S sum_m |w_m val_c[m]| / sqrt(Gy Gx),   D = max_yx 2 / (a_y a_x):
    a cell sums at most M terms, each with the rounded w val, the rounded weight product and the one-unit allowance on
    the two weights; the inverse FFT adds 4 per stage on sum_j |grid_j| <= S sum_m |w val|; the de-apodisation 3."""
    v = _samples_complex(val)
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    M = v.shape[1]
    total = (np.abs(v) * np.abs(_weights_numpy(weights, M))[None, :]).sum(axis=1)
    return (_gamma(M + 2 + 4 + 3 + _fft_roundings(H, W)) * float(_deapodisation(H, W).max()) * _nufft_tap_sum(pos, H, W)
            * total / math.sqrt(4.0 * H * W))


def nufft_scratch_floats(coils: int, H: int, W: int, M: int) -> int:
    return _scratch_query("inr_nufft_scratch", coils, H, W, M)


def nufft_device_apodisation(H: int, W: int, device):
    """(apod_y [H], apod_x [W]) fp32 on the device"""
    return (torch.from_numpy(nufft_apodisation(H)).to(device), torch.from_numpy(nufft_apodisation(W)).to(device))


def nufft_device_bins(pos, H: int, W: int, device):
    """nufft_bins on the device: (bin_start, order) int32 tensors"""
    if isinstance(pos, torch.Tensor):
        pos = pos.detach().cpu().numpy()
    bin_start, order = nufft_bins(pos, H, W)
    return torch.from_numpy(bin_start).to(device), torch.from_numpy(order).to(device)


def nufft(img: torch.Tensor, pos, scratch: Optional[torch.Tensor] = None, apod=None) -> torch.Tensor:
    """[C, M, 2] fp32 on the device: the gridding approximation of nudft(img, pos) -- inr_nufft_prepare, torch.fft
    (evalchain.fft2c of the 2H x 2W grid), inr_nufft_interp, all on the current stream.  ``scratch``: a float32 device
    buffer of at least nufft_scratch_floats(C, H, W, M) entries; ``apod``: nufft_device_apodisation(H, W, device)
    (defaults: made here)."""
    from .evalchain import fft2c
    img = _device_pairs(img, "nufft", "img", "C, H, W", "nufft_numpy is the host-side restatement")
    coils, H, W = (int(v) for v in img.shape[:3])
    p = _device_positions(pos, img.device)
    M = int(p.shape[0])
    if scratch is None:
        scratch = torch.empty(nufft_scratch_floats(coils, H, W, M), device=img.device, dtype=torch.float32)
    ay, ax = apod if apod is not None else nufft_device_apodisation(H, W, img.device)
    grid = torch.empty(coils, 2 * H, 2 * W, 2, device=img.device, dtype=torch.float32)
    out = torch.empty(coils, M, 2, device=img.device, dtype=torch.float32)
    with torch.cuda.device(img.device):  # the FFT between the two calls runs on this device too
        L.launch("inr_nufft_prepare", img.device, img.data_ptr(), ay.data_ptr(), ax.data_ptr(), coils, H, W,
                 grid.data_ptr())
        grid = fft2c(grid).contiguous()
        L.launch("inr_nufft_interp", img.device, grid.data_ptr(), p.data_ptr(), coils, H, W, M, out.data_ptr(),
                 scratch.data_ptr(), scratch.numel())
    return out


def nufft_adjoint(val: torch.Tensor, pos, shape, weights=None, scratch: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, bins=None, apod=None) -> torch.Tensor:
    """[C, H, W, 2] fp32 on the device: the gridding approximation of nudft_adjoint(val, pos, shape, weights) --
    inr_nufft_spread, torch.fft (evalchain.ifft2c of the 2H x 2W grid), inr_nufft_finish, all on the current stream.
    ``bins``: nufft_device_bins(pos, H, W, device) (default: made here, which reads the positions back when they are a
    device tensor); ``scratch``, ``apod``: as for nufft."""
    from .evalchain import ifft2c
    val = _device_pairs(val, "nufft_adjoint", "val", "C, M", "nufft_adjoint_numpy is the host-side restatement")
    coils, M = int(val.shape[0]), int(val.shape[1])
    H, W = (int(v) for v in tuple(shape)[-2:])
    p = _device_positions(pos, val.device)
    if int(p.shape[0]) != M:
        raise ValueError(f"val has {M} samples per coil, pos {int(p.shape[0])}")
    w = _device_weights(weights, M, val.device)
    if scratch is None:
        scratch = torch.empty(nufft_scratch_floats(coils, H, W, M), device=val.device, dtype=torch.float32)
    bin_start, order = bins if bins is not None else nufft_device_bins(pos, H, W, val.device)
    ay, ax = apod if apod is not None else nufft_device_apodisation(H, W, val.device)
    if out is None:
        out = torch.empty(coils, H, W, 2, device=val.device, dtype=torch.float32)
    grid = torch.empty(coils, 2 * H, 2 * W, 2, device=val.device, dtype=torch.float32)
    with torch.cuda.device(val.device):  # the FFT between the two calls runs on this device too
        L.launch("inr_nufft_spread", val.device, val.data_ptr(), p.data_ptr(), None if w is None else w.data_ptr(),
                 bin_start.data_ptr(), order.data_ptr(), coils, H, W, M, grid.data_ptr(), scratch.data_ptr(),
                 scratch.numel())
        grid = ifft2c(grid).contiguous()
        L.launch("inr_nufft_finish", val.device, grid.data_ptr(), ay.data_ptr(), ax.data_ptr(), coils, H, W,
                 out.data_ptr())
    return out


def parse_operator(arg) -> Optional[str]:
    """config['trajectory_operator'] -> None (key absent: the exact operators, nothing recorded), "exact" or "gridding";
    ValueError for anything else"""
    if arg is None:
        return None
    if isinstance(arg, str) and arg in ("exact", "gridding"):
        return arg
    raise ValueError(f"trajectory_operator = {arg!r}: 'exact' or 'gridding'")


# ---- density compensation ----------------------------------------------------------------------------------------------
def normalise_density(w, H: int, W: int) -> np.ndarray:
    """``w`` scaled so that sum w = H W: with the 1/sqrt(H W) of both operators the point-spread function A^H W A then
    has peak 1"""
    w = np.asarray(w, dtype=np.float64)
    return w * (float(H) * float(W) / w.sum())


def density_ramp(n_spokes: int, readout: int, H: Optional[int] = None, W: Optional[int] = None) -> np.ndarray:
    """fp64 [n_spokes * readout], spoke-major: |j - R // 2| for sample j of a spoke and 1/4 for the centre sample (the
    disc of radius half a step, area pi / 4 against the ring's 2 pi |j| / n_spokes per step -- the 1/n_spokes both share
    drops out in the scaling); with H and W, scaled by normalise_density"""
    n_spokes, R = int(n_spokes), int(readout)
    if n_spokes < 1 or R < 2:
        raise ValueError(f"density_ramp: n_spokes = {n_spokes}, readout = {R} (n_spokes >= 1, readout >= 2)")
    w = np.abs(np.arange(R, dtype=np.float64) - R // 2)
    w[R // 2] = 0.25
    w = np.tile(w, n_spokes)
    return w if H is None else normalise_density(w, H, W)


def parse_density(arg, parsed, H: int, W: int):
    """config['trajectory_density'] -> (name, weights fp64 [M] with sum H W) for the parsed trajectory on an H x W grid.
    None / "default": "ramp" for spokes, "uniform" for a file trajectory; "ramp" (spokes only), "uniform", or the path of
    a .npy file of [M] finite positive float64.  ValueError for anything else."""
    if parsed is None:
        raise ValueError("trajectory_density needs a trajectory")
    M = int(positions(parsed, H, W).shape[0])
    if arg is None or (isinstance(arg, str) and arg.lower() in ("default", "none")):
        arg = "ramp" if parsed[0] == "spokes" else "uniform"
    if not isinstance(arg, str):
        raise ValueError(f"trajectory_density = {arg!r}: 'ramp', 'uniform' or the path of a .npy file")
    if arg == "ramp":
        if parsed[0] != "spokes":
            raise ValueError("trajectory_density = 'ramp' needs a spokes trajectory (a file trajectory has no spoke "
                             "structure: give its weights as a .npy file)")
        return "ramp", density_ramp(parsed[1], M // parsed[1], H, W)
    if arg == "uniform":
        return "uniform", normalise_density(np.ones(M, dtype=np.float64), H, W)
    if arg.endswith(".npy"):
        if not os.path.isfile(arg):
            raise ValueError(f"trajectory_density = {arg!r}: no such file")
        w = np.load(arg, allow_pickle=False)
        if w.dtype != np.float64 or w.shape != (M,) or not np.isfinite(w).all() or not (w > 0).all():
            raise ValueError(f"trajectory_density = {arg!r}: expected [{M}] finite positive float64, got {w.dtype} {w.shape}")
        return arg, normalise_density(w, H, W)
    raise ValueError(f"trajectory_density = {arg!r}: 'ramp', 'uniform' or the path of a .npy file")


def parse_baseline(arg):
    """config['trajectory_baseline'] -> None (off), ("adjoint", 0) or ("cg", N), 1 <= N <= 64.  Accepts None / "none",
    "adjoint" and "cg-N"; ValueError for anything else."""
    if arg is None:
        return None
    if isinstance(arg, str):
        if arg.lower() == "none":
            return None
        if arg == "adjoint":
            return ("adjoint", 0)
        m = re.fullmatch(r"cg-(\d+)", arg)
        if m and 1 <= int(m.group(1)) <= 64:
            return ("cg", int(m.group(1)))
    raise ValueError(f"trajectory_baseline = {arg!r}: 'none', 'adjoint' or 'cg-N' with 1 <= N <= 64")


# ---- the conventional reconstruction: conjugate gradients on A^H W A x = A^H W y -----------------------------------------
def _cg(y, w_sum, apply_a, apply_ahw, dot, axpy, iters: int):
    """The iteration both versions run.  ``w_sum(a)``: sum_m w |a|^2; ``dot(a)``: sum |a|^2, both Python floats formed in
    fp64; one alpha and one beta per iteration over all coils.  Returns (iterates, objective)."""
    b = apply_ahw(y)
    if iters == 0:
        return [b], [w_sum(apply_a(b) - y)]
    objective = [w_sum(y)]  # x_0 = 0
    x, s = None, None  # the iterate and A x
    r, p = b, b
    rr = dot(r)
    iterates = []
    for _ in range(iters):
        q = apply_a(p)
        pnp = w_sum(q)  # <p, A^H W A p>
        alpha = rr / pnp if pnp > 0.0 else 0.0
        x = axpy(alpha, p, x)
        s = axpy(alpha, q, s)
        r = axpy(-alpha, apply_ahw(q), r)
        rr_new = dot(r)
        p = axpy(rr_new / rr if rr > 0.0 else 0.0, p, r)
        rr = rr_new
        iterates.append(x)
        objective.append(w_sum(s - y))
    return iterates, objective


def _check_operator(operator: str) -> bool:
    """True for "gridding", False for "exact"; ValueError otherwise"""
    if operator not in ("exact", "gridding"):
        raise ValueError(f"operator = {operator!r}: 'exact' or 'gridding'")
    return operator == "gridding"


def cg_baseline_numpy(values, pos, shape, weights, iters: int, operator: str = "exact"):
    """cg_baseline in fp64 on the host: (iterates [C, H, W] complex128, objective).  ``operator``: "exact" (nudft_numpy
    and its adjoint) or "gridding" (nufft_numpy and its adjoint)."""
    fwd, adj = (nufft_numpy, nufft_adjoint_numpy) if _check_operator(operator) else (nudft_numpy, nudft_adjoint_numpy)
    y = _samples_complex(values)
    H, W = (int(v) for v in tuple(shape)[-2:])
    pos = check_positions(np.asarray(pos, dtype=np.float64))
    w = _weights_numpy(weights, pos.shape[0])
    return _cg(y, lambda a: float((w[None, :] * np.abs(a) ** 2).sum()), lambda x: fwd(x, pos),
               lambda a: adj(a, pos, H, W, w), lambda a: float((np.abs(a) ** 2).sum()),
               lambda k, a, b: k * a if b is None else b + k * a, int(iters))


def cg_baseline(values: torch.Tensor, pos, shape, weights, iters: int, operator: str = "exact"):
    """The density-weighted conjugate-gradient reconstruction of off-grid samples: ``iters`` iterations on
    A^H W A x = A^H W y from x_0 = 0, A = nudft, all coils at once with one alpha and one beta per iteration; the inner
    products are taken with torch on the device, accumulated in fp64, and read back (two scalars per iteration).
    ``values``: [C, M, 2] or [(C*M), 2] fp32 on the device; ``shape`` = (C, H, W); ``weights``: [M] or None.
    Returns (iterates, objective): the image [C, H, W, 2] after each iteration and sum_m w |A x - y|^2 of x_0 = 0 and of
    every iterate (iters + 1 entries, A x carried along the recurrence).  iters = 0: the plain density-weighted adjoint
    A^H W y and its objective.  The two scratch buffers are allocated once.  ``operator`` = "gridding" (DESIGN.md 4.21):
    A = nufft and A^H W = nufft_adjoint instead, with their scratch, bins and apodisation made once."""
    gridding = _check_operator(operator)
    if not isinstance(values, torch.Tensor) or not values.is_cuda:
        raise RuntimeError("cg_baseline only runs on an MI355X (no CPU fallback; cg_baseline_numpy is the host-side version)")
    C_, H, W = (int(v) for v in shape[:3])
    y = values.reshape(C_, -1, 2).contiguous()
    M = int(y.shape[1])
    dev = y.device
    p_dev = _device_positions(pos, dev)
    w32 = _device_weights(weights, M, dev)
    w64 = None if w32 is None else w32.double()
    if gridding:
        taps = torch.empty(nufft_scratch_floats(C_, H, W, M), device=dev, dtype=torch.float32)
        bins, apod = nufft_device_bins(pos, H, W, dev), nufft_device_apodisation(H, W, dev)

        def apply_a(x):
            return nufft(x, p_dev, scratch=taps, apod=apod)

        def apply_ahw(a):
            return nufft_adjoint(a, p_dev, (H, W), w32, scratch=taps, bins=bins, apod=apod)
    else:
        fwd = torch.empty(scratch_floats(C_, H, W, M), device=dev, dtype=torch.float32)
        adj = torch.empty(adjoint_scratch_floats(C_, H, W, M), device=dev, dtype=torch.float32)

        def apply_a(x):
            return nudft(x, p_dev, scratch=fwd)

        def apply_ahw(a):
            return nudft_adjoint(a, p_dev, (H, W), w32, scratch=adj)

    def w_sum(a):
        e = (a.double() ** 2).sum(dim=-1)  # [C, M]
        return float((e if w64 is None else e * w64[None, :]).sum())

    return _cg(y, w_sum, apply_a, apply_ahw, lambda a: float((a.double() ** 2).sum()),
               lambda k, a, b: a * k if b is None else torch.add(b, a, alpha=k), int(iters))


# ---- the switch --------------------------------------------------------------------------------------------------------
def add_trajectory_flag(ap) -> None:
    ap.add_argument("--trajectory", type=str, default=None, metavar="ARG",
                    help="train on off-grid k-space samples: spokes-N, spokes-N-R (golden-angle spokes of R samples) or a "
                         ".npy file of [M,2] float64 index positions (config['trajectory']; none: off)")


def apply_trajectory_flag(config: dict, opts) -> dict:
    if getattr(opts, "trajectory", None) is not None:
        config["trajectory"] = opts.trajectory
    return config


def add_baseline_flags(ap) -> None:
    ap.add_argument("--trajectory-baseline", type=str, default=None, metavar="ARG",
                    help="with --trajectory: also reconstruct the same samples conventionally and report it as "
                         "'gridding': adjoint (density-weighted adjoint) or cg-N (N conjugate-gradient iterations, "
                         "1..64) (config['trajectory_baseline']; none: off)")
    ap.add_argument("--trajectory-density", type=str, default=None, metavar="ARG",
                    help="the baseline's density compensation: ramp (spokes), uniform or a .npy file of [M] positive "
                         "float64 (config['trajectory_density']; default: ramp for spokes, uniform for a file)")
    ap.add_argument("--trajectory-operator", type=str, default=None, metavar="ARG",
                    help="the operator pair inside the baseline -- in train_sense, of the off-grid step itself: exact "
                         "(inr_nudft and its adjoint) or gridding (Kaiser-Bessel gridding around an FFT) "
                         "(config['trajectory_operator']; default: exact, in train_sense gridding)")


def apply_baseline_flags(config: dict, opts) -> dict:
    if getattr(opts, "trajectory_baseline", None) is not None:
        config["trajectory_baseline"] = opts.trajectory_baseline
    if getattr(opts, "trajectory_density", None) is not None:
        config["trajectory_density"] = opts.trajectory_density
    if getattr(opts, "trajectory_operator", None) is not None:
        config["trajectory_operator"] = opts.trajectory_operator
    return config
