"""SENSE fits on CALIBRATED coil maps (no reference counterpart): what every accelerated MRI
acquisition does -- keep a fully sampled centre block of k-space (ACS), estimate smooth coil maps from it once, and
reconstruct with the maps fixed.

    block  = the a x b entries of the centred k-space around (H//2, W//2), times a window          [C,a,b]
    low_c  = ifft2c(zero-padded block_c), evaluated at ANY separable set of positions by a small two-stage DFT
    maps_c = low_c / sqrt(sum_c |low_c|^2)         (zero where the RSS is at or below floor * its maximum)

There is no phase reference: the maps keep the object's low-resolution phase, the image network keeps the rest.

Here: the block and its window, the host's phasor tables (``phasor_table``: float64 with the phase reduced first, rounded
to fp32 -- the kernels hold no sine or cosine), the fp32 numpy text of the three kernels of csrc/inr_sense_calib.hip, bit
for bit (``lowres_numpy``, ``maps_numpy``, ``sense_adjoint_numpy``) with a float64 statement beside each, CG-SENSE in
float64 (``cg_sense_numpy``) and on the device (``cg_sense``), and the ctypes bindings on device tensors.
inr_mi355x/train_sense.py (``sense.maps: calibrated``) and inr_mi355x/reconstruct.py use them.
"""
from __future__ import annotations

import math
import re
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import _ptr, _same_device, _shape
from .sense import _c, _f32, _pairs, fft2c_numpy, place_index, sense_apply, sense_apply_numpy

WINDOWS = ("hann", "none")
CALIB_KEYS = ("size", "window", "floor", "acs")
CALIB_DEFAULTS = {"size": [24, 24], "window": "hann", "floor": 0.0, "acs": True}
FULL_WINDOW = (-1.0, 1.0, -1.0, 1.0)


# ---- settings ----------------------------------------------------------------------------------------------------------
def parse_calib(over, H: Optional[int] = None, W: Optional[int] = None) -> dict:
    """config['sense']['calib'] with its defaults: {'size': [a, b] (each 2..64, at most H and W when given), 'window':
    'hann' | 'none', 'floor': f in [0, 1), 'acs': bool}.  ValueError for anything else."""
    over = over or {}
    if not isinstance(over, dict):
        raise ValueError(f"config['sense']['calib'] is a mapping of {list(CALIB_KEYS)}, got {over!r}")
    unknown = sorted(set(over) - set(CALIB_KEYS))
    if unknown:
        raise ValueError(f"config['sense']['calib'] takes {list(CALIB_KEYS)}, got {unknown}")
    d = dict(CALIB_DEFAULTS, **over)
    size = d["size"]
    if not isinstance(size, (list, tuple)) or len(size) != 2 or any(isinstance(v, bool) or int(v) != v for v in size):
        raise ValueError(f"config['sense']['calib']['size'] = {size!r}: two integers [a, b]")
    a, b = (int(v) for v in size)
    if not (2 <= a <= L.SENSE_CALIB_MAX and 2 <= b <= L.SENSE_CALIB_MAX):
        raise ValueError(f"config['sense']['calib']['size'] = {[a, b]}: each in 2..{L.SENSE_CALIB_MAX}")
    if (H is not None and a > H) or (W is not None and b > W):
        raise ValueError(f"config['sense']['calib']['size'] = {[a, b]} exceeds the grid {H} x {W}")
    if d["window"] not in WINDOWS:
        raise ValueError(f"config['sense']['calib']['window'] = {d['window']!r}: one of {list(WINDOWS)}")
    floor = float(d["floor"])
    if not (0.0 <= floor < 1.0):
        raise ValueError(f"config['sense']['calib']['floor'] = {d['floor']!r}: 0 <= floor < 1")
    if not isinstance(d["acs"], bool):
        raise ValueError(f"config['sense']['calib']['acs'] = {d['acs']!r}: true or false")
    return {"size": [a, b], "window": d["window"], "floor": floor, "acs": d["acs"]}


def parse_sense_baseline(arg) -> Optional[int]:
    """config['sense']['baseline'] -> None (off) or N of 'cg-N', 1 <= N <= 64; ValueError for anything else"""
    if arg is None or (isinstance(arg, str) and arg.lower() == "none"):
        return None
    m = re.fullmatch(r"cg-(\d+)", arg) if isinstance(arg, str) else None
    if m and 1 <= int(m.group(1)) <= 64:
        return int(m.group(1))
    raise ValueError(f"config['sense']['baseline'] = {arg!r}: 'none' or 'cg-N' with 1 <= N <= 64")


# ---- checkpoints (train_sense.py writes them, reconstruct.py reads them) -----------------------------------------------------
def calibrated_state(scale: float, coils_per_step: int, calib: dict, block: torch.Tensor) -> dict:
    """the 'sense' entry of a calibrated-maps checkpoint: the maps themselves are not stored, ``block`` (the windowed
    [C,a,b,2] centre, 69 KB at 15 coils and 24 x 24) rebuilds them on any grid"""
    return {"scale": float(scale), "coils_per_step": int(coils_per_step), "maps": "calibrated",
            "calib": {k: calib[k] for k in CALIB_KEYS}, "block": block.detach().cpu().clone()}


def image_net_state(state_dict: dict):
    """'image.' + the image network's keys (clones): the 'net' of a calibrated-maps checkpoint.  Kept for callers
    outside the package: the trainer writes the same keys through checkpoint.joined_net over its one part."""
    from collections import OrderedDict
    from .sense import IMAGE_PREFIX
    return OrderedDict((IMAGE_PREFIX + k, v.detach().clone()) for k, v in state_dict.items())


def image_net_of(net_state: dict) -> dict:
    """the image network's state_dict of image_net_state's; ValueError when other keys are there"""
    from .sense import IMAGE_PREFIX
    other = [k for k in net_state if not k.startswith(IMAGE_PREFIX)]
    if other or not net_state:
        raise ValueError(f"a calibrated-maps checkpoint holds '{IMAGE_PREFIX}' keys only, got {other[:4]}")
    return {k[len(IMAGE_PREFIX):]: v for k, v in net_state.items()}


def check_sense_mode(theirs: Optional[dict], mode: str) -> None:
    """ValueError unless the checkpoint's 'sense' entry was written under ``mode`` ('learned' | 'calibrated')"""
    got = (theirs or {}).get("maps", "learned")
    if got != mode:
        raise ValueError(f"checkpoint and trainer disagree on config['sense']: maps = {got!r} in the checkpoint, "
                         f"{mode!r} here")


def check_calibrated_state(theirs: dict, mine: dict) -> None:
    """ValueError naming the first of scale / coils_per_step / calib / block on which a checkpoint's 'sense' entry and
    the trainer's differ"""
    check_sense_mode(theirs, "calibrated")
    for key in ("scale", "coils_per_step", "calib"):
        if theirs.get(key) != mine[key]:
            raise ValueError(f"checkpoint and trainer disagree on config['sense']: {key} = {theirs.get(key)!r} in the "
                             f"checkpoint, {mine[key]!r} here")
    blk = theirs.get("block")
    if blk is None or tuple(blk.shape) != tuple(mine["block"].shape) or not torch.equal(blk.cpu(), mine["block"].cpu()):
        raise ValueError("checkpoint and trainer disagree on config['sense']: block (the windowed calibration centre) is "
                         "not the one of the trainer's data")


# ---- the block ---------------------------------------------------------------------------------------------------------
def block_range(N: int, a: int) -> Tuple[int, int]:
    """[r0, r0 + a): the rows (columns) of the centred k-space the block takes, r0 = N//2 - a//2"""
    r0 = N // 2 - a // 2
    if a < 1 or r0 < 0 or r0 + a > N:
        raise ValueError(f"a block of {a} entries does not fit an axis of {N}")
    return r0, r0 + a


def block_mask(H: int, W: int, a: int, b: int) -> np.ndarray:
    """bool [H,W]: True on the block"""
    m = np.zeros((H, W), dtype=bool)
    (r0, r1), (c0, c1) = block_range(H, a), block_range(W, b)
    m[r0:r1, c0:c1] = True
    return m


def add_acs(mask_hw: np.ndarray, a: int, b: int) -> np.ndarray:
    """the [H,W] sampling mask with the block OR-ed in"""
    m = np.asarray(mask_hw) != 0
    return m | block_mask(m.shape[0], m.shape[1], a, b)


def missing_in_block(mask_chw: np.ndarray, a: int, b: int) -> int:
    """entries of the block that the [C,H,W] (or [H,W]) mask does not sample, over all coils"""
    m = np.asarray(mask_chw) != 0
    blk = block_mask(m.shape[-2], m.shape[-1], a, b)
    return int(np.count_nonzero(~m[..., blk]))


def window_1d(a: int, kind: str) -> np.ndarray:
    """float64 [a]: the window along one axis of the block, 1 at the block's DC entry (index a//2).  'hann':
    cos^2(pi (i - a//2) / (a + 1)) -- a raised cosine whose zeros lie outside the block, so that no measured entry is
    thrown away; 'none': ones."""
    if kind not in WINDOWS:
        raise ValueError(f"window = {kind!r}: one of {list(WINDOWS)}")
    if kind == "none":
        return np.ones(a, dtype=np.float64)
    return np.cos(np.pi * (np.arange(a, dtype=np.float64) - a // 2) / (a + 1)) ** 2


def cut_block(kspace, a: int, b: int, window: str = "hann") -> np.ndarray:
    """fp32 [C,a,b,2]: the block of the centred k-space [C,H,W,2] (numpy or torch), times the separable window.  The
    product is formed in float64 and rounded once."""
    k = kspace.detach().cpu().numpy() if isinstance(kspace, torch.Tensor) else np.asarray(kspace)
    if k.ndim != 4 or k.shape[-1] != 2:
        raise ValueError(f"kspace has shape {k.shape}, expected [C,H,W,2]")
    (r0, r1), (c0, c1) = block_range(k.shape[1], a), block_range(k.shape[2], b)
    w = window_1d(a, window)[:, None] * window_1d(b, window)[None, :]
    return np.ascontiguousarray((k[:, r0:r1, c0:c1].astype(np.float64) * w[None, :, :, None]).astype(np.float32))


# ---- positions and phasor tables ---------------------------------------------------------------------------------------
def axis_positions(N: int, n: int, lo: float = -1.0, hi: float = 1.0) -> np.ndarray:
    """float64 [n]: pixel positions (in units of the fit's own pixels, 0 .. N-1 over the window -1 .. 1) of ``n`` points
    spread over [lo, hi] as grid.py spreads them; exact integers on the fit's own grid."""
    if n == N and lo == -1.0 and hi == 1.0:
        return np.arange(N, dtype=np.float64)
    i = np.arange(n, dtype=np.float64)
    c = lo + (hi - lo) * (i / (n - 1)) if n > 1 else np.full(1, lo, dtype=np.float64)
    return (c + 1.0) * 0.5 * (N - 1)


def block_index(N: int, a: int) -> np.ndarray:
    """int64 [a]: the frequency index k - N//2 of every block entry along an axis of N"""
    r0, r1 = block_range(N, a)
    return np.arange(r0, r1, dtype=np.int64) - N // 2


def phasor_table_float64(idx, pos, N: int) -> np.ndarray:
    """complex128 [a,n]: exp(2 pi i k (p - N//2) / N) / sqrt(N) for the frequency indices ``idx`` and the pixel positions
    ``pos``: the row of the centred orthonormal inverse transform.  The phase is reduced before the sine and cosine:
    k (p - N//2) is formed in float64 (exact for integer positions), taken modulo N (fmod is exact), and only the
    remainder is scaled by 2 pi / N."""
    k = np.asarray(idx, dtype=np.float64)[:, None]
    p = np.asarray(pos, dtype=np.float64)[None, :] - float(N // 2)
    r = np.fmod(k * p, float(N))
    ang = (2.0 * np.pi / N) * r
    return (np.cos(ang) + 1j * np.sin(ang)) / math.sqrt(N)


def phasor_table(idx, pos, N: int) -> np.ndarray:
    """fp32 [a,n,2]: phasor_table_float64 rounded to fp32 -- what inr_sense_lowres reads as ey / ex"""
    return np.ascontiguousarray(_pairs(phasor_table_float64(idx, pos, N)).astype(np.float32))


def grid_tables(H: int, W: int, a: int, b: int, Ho: Optional[int] = None, Wo: Optional[int] = None,
                window: Sequence[float] = FULL_WINDOW) -> Tuple[np.ndarray, np.ndarray]:
    """(ey [a,Ho,2], ex [b,Wo,2]) fp32 for a rendering of Ho x Wo points over ``window`` = (y0, y1, x0, x1) of a fit on
    H x W; default: the fit's own grid"""
    Ho, Wo = int(Ho or H), int(Wo or W)
    y0, y1, x0, x1 = (float(v) for v in window)
    return (phasor_table(block_index(H, a), axis_positions(H, Ho, y0, y1), H),
            phasor_table(block_index(W, b), axis_positions(W, Wo, x0, x1), W))


# ---- the three kernels in numpy ----------------------------------------------------------------------------------------
def lowres_float64(kc, ey, ex) -> np.ndarray:
    """complex128 [C,Ho,Wo]: out[c,y,x] = sum_j ey[j,y] sum_i kc[c,j,i] ex[i,x] of complex (or (re, im)) arrays"""
    cx = lambda v: _c(np.asarray(v, dtype=np.float64)) if not np.iscomplexobj(v) else np.asarray(v, dtype=np.complex128)
    return np.einsum("jy,cji,ix->cyx", cx(ey), cx(kc), cx(ex))


def _cmul_add(ur, ui, vr, vi, sr, si):
    p0, p1, p2, p3 = ur * vr, ui * vi, ur * vi, ui * vr
    return sr + (p0 - p1), si + (p2 + p3)


def lowres_numpy(kc, ey, ex) -> np.ndarray:
    """fp32 [C,Ho,Wo,2]: the text of inr_sense_lowres -- T summed over i ascending, out over j ascending, both from zero,
    every product, difference and sum one fp32 operation"""
    kc, ey, ex = (np.ascontiguousarray(v, dtype=np.float32) for v in (kc, ey, ex))
    C, a, b = kc.shape[:3]
    Ho, Wo = ey.shape[1], ex.shape[1]
    Tr, Ti = np.zeros((C, a, Wo), np.float32), np.zeros((C, a, Wo), np.float32)
    for i in range(b):
        Tr, Ti = _cmul_add(kc[:, :, i, 0, None], kc[:, :, i, 1, None], ex[None, None, i, :, 0], ex[None, None, i, :, 1],
                           Tr, Ti)
    outr, outi = np.zeros((C, Ho, Wo), np.float32), np.zeros((C, Ho, Wo), np.float32)
    for j in range(a):
        outr, outi = _cmul_add(ey[None, j, :, 0, None], ey[None, j, :, 1, None], Tr[:, j, None, :], Ti[:, j, None, :],
                               outr, outi)
    return np.stack((outr, outi), axis=-1)


def maps_float64(low, floor: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """(maps complex128 [C,...], rss float64 [...]) of complex (or (re, im)) low-resolution coil images"""
    z = _c(np.asarray(low, dtype=np.float64)) if not np.iscomplexobj(low) else np.asarray(low, dtype=np.complex128)
    rss = np.sqrt((np.abs(z) ** 2).sum(axis=0))
    keep = (rss > floor * rss.max()) & (rss > 0)
    return np.where(keep[None], z / np.where(keep, rss, 1.0)[None], 0.0), rss


def maps_numpy(low, C: int, P: int, floor: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """(maps [C,P,2], rss [P]) fp32: the text of inr_sense_maps"""
    low, f = _f32(low, C, P, 2), np.float32(floor)
    r2 = np.zeros(P, dtype=np.float32)
    for c in range(C):
        r2 = r2 + (low[c, :, 0] * low[c, :, 0] + low[c, :, 1] * low[c, :, 1])
    rss = np.sqrt(r2)
    thr = f * np.fmax.reduce(rss, initial=np.float32(0.0)) if f > 0 else np.float32(0.0)
    keep = (rss > thr) & (rss > 0)
    maps = np.zeros((C, P, 2), dtype=np.float32)
    maps[:, keep] = low[:, keep] / rss[None, keep, None]
    return maps, rss


def sense_adjoint_numpy(sens, gx, G: int, H: int, W: int, scale: float, shift: int) -> np.ndarray:
    """dimg [H*W,2] fp32: the text of inr_sense_adjoint -- sense_grad_numpy's dimg lines alone"""
    sens, s = _f32(sens, G, H * W, 2), np.float32(scale)
    g = _f32(gx, G, H * W, 2)[:, place_index(H, W) if shift else np.arange(H * W)]
    dimg = np.zeros((H * W, 2), dtype=np.float32)
    for k in range(G):
        ur, ui = s * g[k, :, 0], s * g[k, :, 1]
        sr, si = sens[k, :, 0], sens[k, :, 1]
        dimg[:, 0] = dimg[:, 0] + (sr * ur + si * ui)
        dimg[:, 1] = dimg[:, 1] + (sr * ui - si * ur)
    return dimg


def sense_adjoint_float64(sens, gx, G: int, H: int, W: int, scale: float) -> np.ndarray:
    """complex128 [H,W]: scale * sum_g conj(S_g) gX_g, nothing shifted"""
    S = _c(np.asarray(sens, dtype=np.float64).reshape(G, H, W, 2))
    return scale * np.sum(np.conj(S) * _c(np.asarray(gx, dtype=np.float64).reshape(G, H, W, 2)), axis=0)


def calibrate_numpy(block, H: int, W: int, floor: float = 0.0, Ho=None, Wo=None, window=FULL_WINDOW, fp32: bool = False):
    """(maps, rss) of a windowed block [C,a,b,2] on a grid: float64 (complex [C,Ho,Wo], [Ho,Wo]) from the float64 tables,
    or with ``fp32`` the kernels' own text ([C,Ho*Wo,2], [Ho*Wo]) from the rounded ones"""
    C, a, b = np.asarray(block).shape[:3]
    Ho, Wo = int(Ho or H), int(Wo or W)
    if fp32:
        ey, ex = grid_tables(H, W, a, b, Ho, Wo, window)
        return maps_numpy(lowres_numpy(block, ey, ex), C, Ho * Wo, floor)
    y0, y1, x0, x1 = (float(v) for v in window)
    ey = phasor_table_float64(block_index(H, a), axis_positions(H, Ho, y0, y1), H)
    ex = phasor_table_float64(block_index(W, b), axis_positions(W, Wo, x0, x1), W)
    return maps_float64(lowres_float64(block, ey, ex), floor)


# ---- CG-SENSE ----------------------------------------------------------------------------------------------------------
def _cg_normal(b, normal, dot, axpy, objective, iters: int):
    """``iters`` conjugate-gradient iterations on normal(x) = b from x_0 = 0: (iterates, objective of x_0 and of every
    iterate).  ``dot(u)``: sum |u|^2 as a Python float formed in fp64; ``axpy(k, u, v)``: v + k u (k u when v is None)."""
    obj = [objective(None)]
    x, r, p = None, b, b
    rr = dot(r)
    iterates = []
    for _ in range(iters):
        q, pq = normal(p)
        alpha = rr / pq if pq > 0.0 else 0.0
        x = axpy(alpha, p, x)
        r = axpy(-alpha, q, r)
        rr_new = dot(r)
        p = axpy(rr_new / rr if rr > 0.0 else 0.0, p, r)
        rr = rr_new
        iterates.append(x)
        obj.append(objective(x))
    return iterates, obj


def cg_sense_numpy(maps, y, mask, iters: int, lam: float = 0.0, fp32: bool = False):
    """CG-SENSE on the host: ``iters`` iterations on (sum_c S_c^H F^H M F S_c + lam) x = sum_c S_c^H F^H M y from
    x_0 = 0.  maps: complex [C,H,W]; y: complex centred k-space [C,H,W] (entries outside the mask are ignored); mask:
    [C,H,W] or [H,W] (None: everything sampled).  Returns (iterates complex [H,W], objective): |M (F S x - y)|^2 +
    lam |x|^2 of x_0 = 0 and of every iterate.  float64 throughout; ``fp32``: the same iterations with the fp32 numpy
    operators (sense_apply_numpy, a complex64 FFT, sense_adjoint_numpy) and the scalars in float64 -- what the device
    does with rocFFT in place of this FFT."""
    S = np.asarray(maps, dtype=np.complex128)
    C, H, W = S.shape
    M = np.ones((C, H, W)) if mask is None else np.broadcast_to((np.asarray(mask) != 0).astype(np.float64), (C, H, W))
    y = np.asarray(y, dtype=np.complex128) * M
    if fp32:
        S32 = _pairs(S).astype(np.float32).reshape(C * H * W, 2)
        M32, y = M.astype(np.float32), y.astype(np.complex64)

        def fwd(x):
            X = sense_apply_numpy(_pairs(x).reshape(H * W, 2), S32, C, H, W, 1.0, 0)
            return (fft2c_numpy((X[..., 0] + 1j * X[..., 1]).astype(np.complex64)).astype(np.complex64) * M32)

        def adj(k):
            g = fft2c_numpy((k * M32).astype(np.complex64), inverse=True).astype(np.complex64)
            d = sense_adjoint_numpy(S32, _pairs(g).astype(np.float32), C, H, W, 1.0, 0).reshape(H, W, 2)
            return (d[..., 0] + 1j * d[..., 1]).astype(np.complex64)

        cast = lambda v: v.astype(np.complex64)
    else:
        fwd = lambda x: fft2c_numpy(S * x[None]) * M
        adj = lambda k: np.sum(np.conj(S) * fft2c_numpy(k * M, inverse=True), axis=0)
        cast = lambda v: v
    dot = lambda u: float((np.abs(u.astype(np.complex128)) ** 2).sum())

    def normal(p):
        Ap = fwd(p)
        q = cast(adj(Ap) + lam * p) if lam else adj(Ap)
        return q, dot(Ap) + lam * dot(p)

    def objective(x):
        return dot(y) if x is None else dot(fwd(x) - y) + lam * dot(x)

    axpy = lambda k, u, v: cast(k * u) if v is None else cast(v + k * u)
    return _cg_normal(adj(y), normal, dot, axpy, objective, int(iters))


# ---- the kernels -------------------------------------------------------------------------------------------------------
def sense_lowres(kc: torch.Tensor, ey: torch.Tensor, ex: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_sense_lowres on device tensors kc [C,a,b,2], ey [a,Ho,2], ex [b,Wo,2] -> out [C,Ho,Wo,2]"""
    if kc.dim() != 4 or ey.dim() != 3 or ex.dim() != 3:
        raise RuntimeError(f"kc / ey / ex have shape {tuple(kc.shape)} / {tuple(ey.shape)} / {tuple(ex.shape)}, expected "
                           "[C,a,b,2] / [a,Ho,2] / [b,Wo,2]")
    C, a, b = (int(v) for v in kc.shape[:3])
    Ho, Wo = int(ey.shape[1]), int(ex.shape[1])
    _shape(kc, "kc", C, a, b, 2)
    _shape(ey, "ey", a, Ho, 2)
    _shape(ex, "ex", b, Wo, 2)
    out = torch.empty(C, Ho, Wo, 2, device=kc.device) if out is None else out
    _shape(out, "out", C, Ho, Wo, 2)
    ptrs = (_ptr(kc, "kc"), _ptr(ey, "ey"), _ptr(ex, "ex"), _ptr(out, "out"))
    _same_device(kc, ey=ey, ex=ex, out=out)
    L.launch("inr_sense_lowres", kc.device, ptrs[0], ptrs[1], ptrs[2], C, a, b, Ho, Wo, ptrs[3])
    return out


def sense_maps(low: torch.Tensor, C: int, P: int, floor: float = 0.0, maps: Optional[torch.Tensor] = None,
               rss: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """inr_sense_maps on a device tensor low [C,P,2] (any shape of C*P*2 entries laid out so) -> (maps [C,P,2], rss [P])"""
    low = low.view(C, P, 2)
    _shape(low, "low", C, P, 2)
    maps = torch.empty(C, P, 2, device=low.device) if maps is None else maps
    rss = torch.empty(P, device=low.device) if rss is None else rss
    _shape(maps, "maps", C, P, 2)
    _shape(rss, "rss", P)
    ptrs = (_ptr(low, "low"), _ptr(maps, "maps"), _ptr(rss, "rss"))
    _same_device(low, maps=maps, rss=rss)
    L.launch("inr_sense_maps", low.device, ptrs[0], C, P, float(floor), ptrs[1], ptrs[2])
    return maps, rss


def sense_adjoint(sens: torch.Tensor, gx: torch.Tensor, G: int, H: int, W: int, scale: float, shift: int = 1,
                  dimg: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_sense_adjoint on device tensors sens [G*H*W,2], gx [G,H,W,2] -> dimg [H*W,2]"""
    _shape(sens, "sens", G * H * W, 2)
    _shape(gx, "gx", G, H, W, 2)
    dimg = torch.empty(H * W, 2, device=sens.device) if dimg is None else dimg
    _shape(dimg, "dimg", H * W, 2)
    ptrs = (_ptr(sens, "sens"), _ptr(gx, "gx"), _ptr(dimg, "dimg"))
    _same_device(sens, gx=gx, dimg=dimg)
    L.launch("inr_sense_adjoint", sens.device, ptrs[0], ptrs[1], G, H, W, float(scale), int(shift), ptrs[2])
    return dimg


def calibrate(block: torch.Tensor, H: int, W: int, floor: float = 0.0, Ho: Optional[int] = None, Wo: Optional[int] = None,
              window: Sequence[float] = FULL_WINDOW) -> Tuple[torch.Tensor, torch.Tensor]:
    """(maps [C,Ho*Wo,2], rss [Ho*Wo]) on the device from the windowed block [C,a,b,2] of a fit on H x W: the host's two
    phasor tables, inr_sense_lowres, inr_sense_maps.  Default grid: the fit's own."""
    C, a, b = (int(v) for v in block.shape[:3])
    Ho, Wo = int(Ho or H), int(Wo or W)
    ey, ex = (torch.from_numpy(t).to(block.device) for t in grid_tables(H, W, a, b, Ho, Wo, window))
    low = sense_lowres(block.contiguous(), ey, ex)
    return sense_maps(low, C, Ho * Wo, floor)


@torch.no_grad()
def cg_sense(maps: torch.Tensor, y_s: torch.Tensor, mask_s: Optional[torch.Tensor], shape, iters: int, lam: float = 0.0):
    """CG-SENSE on the device (cg_sense_numpy's iterations): inr_sense_apply(scale 1, shift 1) gives S x where ifftshift
    puts it, torch.fft the transforms, a multiply the mask, inr_sense_adjoint sum_c S_c^H.  maps [C,H*W,2]; y_s
    [C*H*W,2] and mask_s [C*H*W] (or None) in the ifftshift-ed row order of the trainer's ingest.  The inner products are
    formed in fp64 on the device and read back (two scalars per iteration).  Returns (iterates [H*W,2], objective)."""
    C, H, W = (int(v) for v in shape[:3])
    P = H * W
    sens = maps.reshape(C * P, 2)
    m = None if mask_s is None else mask_s.view(C, H, W, 1).to(torch.float32)
    y = y_s.view(C, H, W, 2) if m is None else y_s.view(C, H, W, 2) * m
    xbuf = torch.empty(C, H, W, 2, device=maps.device)

    def fwd(x):
        X = sense_apply(x.contiguous(), sens, C, H, W, 1.0, 1, out=xbuf)
        k = torch.view_as_real(torch.fft.fft2(torch.view_as_complex(X), norm="ortho"))
        return k if m is None else k * m

    def adj(k):
        k = k if m is None else k * m
        g = torch.view_as_real(torch.fft.ifft2(torch.view_as_complex(k.contiguous()), norm="ortho")).contiguous()
        return sense_adjoint(sens, g, C, H, W, 1.0, 1)

    dot = lambda u: float((u.double() ** 2).sum())

    def normal(p):
        Ap = fwd(p)
        q = adj(Ap)
        return (q + lam * p if lam else q), dot(Ap) + lam * dot(p)

    def objective(x):
        return dot(y) if x is None else dot(fwd(x) - y) + lam * dot(x)

    axpy = lambda k, u, v: k * u if v is None else v + k * u
    return _cg_normal(adj(y), normal, dot, axpy, objective, int(iters))


def kspace_of(x: torch.Tensor, maps: torch.Tensor, shape, scale: float = 1.0) -> torch.Tensor:
    """[C*H*W,2]: the centred k-space of the image x [H*W,2] through the maps, in the dataset's own order"""
    C, H, W = (int(v) for v in shape[:3])
    X = sense_apply(x.contiguous(), maps.reshape(C * H * W, 2), C, H, W, scale, 1)
    k = torch.fft.fftshift(torch.fft.fft2(torch.view_as_complex(X), norm="ortho"), dim=(-2, -1))
    return torch.view_as_real(k).reshape(-1, 2).contiguous()
