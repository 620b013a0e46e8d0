"""Off-grid SENSE fits on calibrated maps (no reference counterpart): the operator between an
image network and off-grid multi-coil samples, and its conjugate transpose,

    E x   = nufft(scale * S_g * x)              [G, M]      (trajectory.nufft's gridding approximation of the NUDFT)
    E^H k = scale * sum_g conj(S_g) nufft_adjoint(w * k_g)  [H, W]

each as one fused kernel, a PLAIN torch.fft on the twice oversampled grid, and one gather kernel:

    sense_nufft          inr_sense_nufft_prepare -> torch.fft.fft2(ortho)  -> inr_nufft_interp_plain
    sense_nufft_adjoint  inr_nufft_spread_plain  -> torch.fft.ifft2(ortho) -> inr_sense_nufft_finish

The grid is kept in the layout a plain FFT reads and writes: the centred grid of trajectory.nufft rolled by (H, W) --
2H and 2W are even, so fftshift and ifftshift are that one roll (``plain_roll``).  No coil images, no fftshift / ifftshift
and no .contiguous() copy exist between the network and the samples.

Here: the fp32 numpy text of the two fused kernels, bit for bit (``sense_nufft_prepare_numpy``,
``sense_nufft_finish_numpy``), the float64 statement of both operators on trajectory.nufft_numpy / nufft_adjoint_numpy
(``sense_nufft_numpy``, ``sense_nufft_adjoint_numpy``), non-Cartesian CG-SENSE on them (``cg_sense_nufft_numpy``, and
``cg_sense_offgrid`` on the device), and the ctypes bindings on device tensors.  inr_mi355x/train_sense.py
(``sense.maps: calibrated`` with ``trajectory``) uses them.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import trajectory as T
from .engine import _ptr, _same_device, _shape
from .sense import _c, _f32, _pairs


# ---- the layout ----------------------------------------------------------------------------------------------------------
def plain_roll(grid, H: int, W: int):
    """the centred [..., 2H, 2W(, 2)] grid in plain layout, or back: the roll by (H, W) over the two grid axes (its own
    inverse).  numpy arrays and tensors; a trailing axis of 2 holds (re, im) pairs."""
    pairs = grid.shape[-1] == 2 and grid.ndim >= 3 and grid.shape[-2] == 2 * W
    axes = (-3, -2) if pairs else (-2, -1)
    if isinstance(grid, torch.Tensor):
        return torch.roll(grid, (H, W), axes)
    return np.roll(grid, (H, W), axes)


def _deapodisation_f32(H: int, W: int) -> np.ndarray:
    """fp32 [H, W]: the kernels' deapodise, 2 / (a_y * a_x) with one rounded product and one rounded division"""
    ay, ax = T.nufft_apodisation(H), T.nufft_apodisation(W)
    return np.float32(2.0) / (ay[:, None] * ax[None, :])


def _centre(H: int, W: int):
    """the slices of the CENTRED grid that hold the image"""
    y0, x0 = H - H // 2, W - W // 2
    return slice(y0, y0 + H), slice(x0, x0 + W)


# ---- the two fused kernels in fp32 numpy ---------------------------------------------------------------------------------
def sense_nufft_prepare_numpy(img, maps, G: int, H: int, W: int, scale: float) -> np.ndarray:
    """grid [G, 2H, 2W, 2] fp32 in plain layout: the text of inr_sense_nufft_prepare -- inr_sense_apply's product, then one
    rounded multiplication by 2 / (a_y a_x) per component, zeros in the padding"""
    T._nufft_check_shape(H, W)
    img, maps, s = _f32(img, H * W, 2), _f32(maps, G, H * W, 2), np.float32(scale)
    ir, ii = img[None, :, 0], img[None, :, 1]
    sr, si = maps[..., 0], maps[..., 1]
    re = sr * ir - si * ii
    im = sr * ii + si * ir
    d = _deapodisation_f32(H, W).reshape(1, H * W)
    grid = np.zeros((G, 2 * H, 2 * W, 2), dtype=np.float32)
    ys, xs = _centre(H, W)
    grid[:, ys, xs, 0] = ((s * re) * d).reshape(G, H, W)
    grid[:, ys, xs, 1] = ((s * im) * d).reshape(G, H, W)
    return plain_roll(grid, H, W)


def sense_nufft_finish_numpy(grid, maps, G: int, H: int, W: int, scale: float, dimg=None) -> np.ndarray:
    """dimg [H*W, 2] fp32: the text of inr_sense_nufft_finish on a plain-layout grid [G, 2H, 2W, 2] -- the centre cell times
    2 / (a_y a_x), inr_sense_adjoint's lines, summed from zero in coil order; ``dimg``: what accumulate = 1 adds to"""
    T._nufft_check_shape(H, W)
    maps, s = _f32(maps, G, H * W, 2), np.float32(scale)
    ys, xs = _centre(H, W)
    g = plain_roll(_f32(grid, G, 2 * H, 2 * W, 2), H, W)[:, ys, xs]
    d = _deapodisation_f32(H, W)[None, :, :, None]
    v = (g * d).reshape(G, H * W, 2)
    acc = np.zeros((H * W, 2), dtype=np.float32)
    for k in range(G):
        ur, ui = s * v[k, :, 0], s * v[k, :, 1]
        sr, si = maps[k, :, 0], maps[k, :, 1]
        acc[:, 0] = acc[:, 0] + (sr * ur + si * ui)
        acc[:, 1] = acc[:, 1] + (sr * ui - si * ur)
    return acc if dimg is None else _f32(dimg, H * W, 2) + acc


# ---- the two operators in float64 ----------------------------------------------------------------------------------------
def _maps_complex(maps, G: int, H: int, W: int) -> np.ndarray:
    m = np.asarray(maps)
    if np.iscomplexobj(m):
        return m.astype(np.complex128).reshape(G, H, W)
    return _c(m.astype(np.float64).reshape(G, H, W, 2))


def sense_nufft_numpy(img, maps, pos, G: int, H: int, W: int, scale: float) -> np.ndarray:
    """[G, M] complex128: nufft_numpy of the coil images scale * S_g * I.  img [H*W, 2] pairs or complex [H, W]; maps
    [G, H*W, 2] pairs or complex [G, H, W]."""
    I = np.asarray(img)
    I = I.astype(np.complex128).reshape(H, W) if np.iscomplexobj(I) else _c(I.astype(np.float64).reshape(H, W, 2))
    return T.nufft_numpy(scale * _maps_complex(maps, G, H, W) * I[None], pos)


def sense_nufft_adjoint_numpy(gk, maps, pos, G: int, H: int, W: int, scale: float, weights=None) -> np.ndarray:
    """[H, W] complex128: scale * sum_g conj(S_g) nufft_adjoint_numpy(weights * gk_g) -- the exact conjugate transpose of
    sense_nufft_numpy (times the weights).  gk: [G, M, 2] pairs or complex [G, M]."""
    back = T.nufft_adjoint_numpy(gk, pos, H, W, weights)
    return scale * np.sum(np.conj(_maps_complex(maps, G, H, W)) * back, axis=0)


# ---- non-Cartesian CG-SENSE (Pruessmann 2001) ------------------------------------------------------------------------------
def cg_sense_nufft_numpy(maps, y, pos, weights, iters: int, lam: float = 0.0, fp32: bool = False):
    """``iters`` conjugate-gradient iterations on (E^H W E + lam) x = E^H W y from x_0 = 0, E = sense_nufft_numpy with
    scale 1: (iterates complex [H, W], objective sum_m w |E x - y|^2 + lam |x|^2 of x_0 = 0 and of every iterate).
    maps: complex [G, H, W]; y: complex [G, M].  float64 throughout; ``fp32``: the same iterations with the operands of
    every operator call and the iterates rounded to complex64 and the two fused kernels in their fp32 text (the FFT a
    complex64 one, taps and sums in float64) -- an estimate of what the device's rounding does to the iterations."""
    from .sense_calib import _cg_normal
    S = np.asarray(maps, dtype=np.complex128)
    G, H, W = S.shape
    pos = T.check_positions(np.asarray(pos, dtype=np.float64))
    w = T._weights_numpy(weights, pos.shape[0])
    y = np.asarray(y, dtype=np.complex128)
    if fp32:
        S32 = _pairs(S).astype(np.float32).reshape(G, H * W, 2)
        iy, ix, wy, wx = T._nufft_cells(pos, H, W)
        y = y.astype(np.complex64)

        def fwd(x):
            g = plain_roll(sense_nufft_prepare_numpy(_pairs(x).reshape(H * W, 2), S32, G, H, W, 1.0), H, W)
            k = T._fftc_numpy(_c(g).astype(np.complex64), False).astype(np.complex64)
            return np.einsum("cmyx,my,mx->cm", k[:, iy[:, :, None], ix[:, None, :]], wy, wx).astype(np.complex64)

        def adj(k):
            v = (k * w[None, :]).astype(np.complex64)
            grid = np.zeros((G, 2 * H, 2 * W), dtype=np.complex128)
            contrib = v[:, :, None, None] * (wy[:, :, None] * wx[:, None, :])[None]
            for c in range(G):
                np.add.at(grid[c], (np.broadcast_to(iy[:, :, None], contrib.shape[1:]),
                                    np.broadcast_to(ix[:, None, :], contrib.shape[1:])), contrib[c])
            g = T._fftc_numpy(grid.astype(np.complex64), True).astype(np.complex64)
            d = sense_nufft_finish_numpy(plain_roll(_pairs(g).astype(np.float32), H, W), S32, G, H, W, 1.0)
            return _c(d.reshape(H, W, 2)).astype(np.complex64)

        cast = lambda v: v.astype(np.complex64)
    else:
        fwd = lambda x: sense_nufft_numpy(x, S, pos, G, H, W, 1.0)
        adj = lambda k: sense_nufft_adjoint_numpy(k, S, pos, G, H, W, 1.0, w)
        cast = lambda v: v
    dot = lambda u: float((np.abs(u.astype(np.complex128)) ** 2).sum())
    w_sum = lambda a: float((w[None, :] * np.abs(a.astype(np.complex128)) ** 2).sum())

    def normal(p):
        Ep = fwd(p)
        q = adj(Ep)
        return (cast(q + lam * p) if lam else q), w_sum(Ep) + lam * dot(p)

    def objective(x):
        return w_sum(y) if x is None else w_sum(fwd(x) - y) + lam * dot(x)

    axpy = lambda k, u, v: cast(k * u) if v is None else cast(v + k * u)
    return _cg_normal(adj(y), normal, dot, axpy, objective, int(iters))


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _apod(apod, H: int, W: int, device):
    ay, ax = apod if apod is not None else T.nufft_device_apodisation(H, W, device)
    _shape(ay, "apod_y", H)
    _shape(ax, "apod_x", W)
    return ay, ax


def sense_nufft_prepare(img: torch.Tensor, maps: torch.Tensor, G: int, H: int, W: int, scale: float, apod=None,
                        grid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_sense_nufft_prepare on device tensors img [H*W,2], maps [G*H*W,2] -> grid [G,2H,2W,2] in plain layout"""
    _shape(img, "img", H * W, 2)
    _shape(maps, "maps", G * H * W, 2)
    ay, ax = _apod(apod, H, W, img.device)
    grid = torch.empty(G, 2 * H, 2 * W, 2, device=img.device) if grid is None else grid
    _shape(grid, "grid", G, 2 * H, 2 * W, 2)
    ptrs = (_ptr(img, "img"), _ptr(maps, "maps"), _ptr(ay, "apod_y"), _ptr(ax, "apod_x"), _ptr(grid, "grid"))
    _same_device(img, maps=maps, apod_y=ay, apod_x=ax, grid=grid)
    L.launch("inr_sense_nufft_prepare", img.device, ptrs[0], ptrs[1], ptrs[2], ptrs[3], G, H, W, float(scale), ptrs[4])
    return grid


def sense_nufft_finish(grid: torch.Tensor, maps: torch.Tensor, G: int, H: int, W: int, scale: float, apod=None,
                       dimg: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """inr_sense_nufft_finish on device tensors grid [G,2H,2W,2] (plain layout), maps [G*H*W,2] -> dimg [H*W,2], written
    or, with ``accumulate``, added to"""
    _shape(grid, "grid", G, 2 * H, 2 * W, 2)
    _shape(maps, "maps", G * H * W, 2)
    ay, ax = _apod(apod, H, W, grid.device)
    if dimg is None:
        if accumulate:
            raise ValueError("sense_nufft_finish: accumulate needs a dimg to add to")
        dimg = torch.empty(H * W, 2, device=grid.device)
    _shape(dimg, "dimg", H * W, 2)
    ptrs = (_ptr(grid, "grid"), _ptr(maps, "maps"), _ptr(ay, "apod_y"), _ptr(ax, "apod_x"), _ptr(dimg, "dimg"))
    _same_device(grid, maps=maps, apod_y=ay, apod_x=ax, dimg=dimg)
    L.launch("inr_sense_nufft_finish", grid.device, ptrs[0], ptrs[1], ptrs[2], ptrs[3], G, H, W, float(scale), ptrs[4],
             int(bool(accumulate)))
    return dimg


def _scratch(scratch, G: int, H: int, W: int, M: int, device) -> torch.Tensor:
    if scratch is None:
        return torch.empty(T.nufft_scratch_floats(G, H, W, M), device=device, dtype=torch.float32)
    return scratch


def nufft_interp_plain(grid: torch.Tensor, pos: torch.Tensor, G: int, H: int, W: int, scratch=None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_nufft_interp_plain: grid [G,2H,2W,2] in plain layout, pos [M,2] fp64 on the device -> out [G,M,2]"""
    _shape(grid, "grid", G, 2 * H, 2 * W, 2)
    M = int(pos.shape[0])
    scratch = _scratch(scratch, G, H, W, M, grid.device)
    out = torch.empty(G, M, 2, device=grid.device) if out is None else out
    _shape(out, "out", G, M, 2)
    _same_device(grid, pos=pos, out=out, scratch=scratch)
    L.launch("inr_nufft_interp_plain", grid.device, _ptr(grid, "grid"), pos.data_ptr(), G, H, W, M, _ptr(out, "out"),
             scratch.data_ptr(), scratch.numel())
    return out


def nufft_spread_plain(val: torch.Tensor, pos: torch.Tensor, weights, bins, G: int, H: int, W: int, scratch=None,
                       grid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_nufft_spread_plain: val [G,M,2], pos [M,2] fp64, weights [M] fp32 or None, bins = nufft_device_bins(...), all
    on the device -> grid [G,2H,2W,2] in plain layout, every cell written"""
    M = int(pos.shape[0])
    _shape(val, "val", G, M, 2)
    scratch = _scratch(scratch, G, H, W, M, val.device)
    grid = torch.empty(G, 2 * H, 2 * W, 2, device=val.device) if grid is None else grid
    _shape(grid, "grid", G, 2 * H, 2 * W, 2)
    bin_start, order = bins
    _same_device(val, pos=pos, grid=grid, scratch=scratch, bin_start=bin_start, order=order)
    L.launch("inr_nufft_spread_plain", val.device, _ptr(val, "val"), pos.data_ptr(),
             None if weights is None else weights.data_ptr(), bin_start.data_ptr(), order.data_ptr(), G, H, W, M,
             _ptr(grid, "grid"), scratch.data_ptr(), scratch.numel())
    return grid


def sense_nufft(img: torch.Tensor, maps: torch.Tensor, pos, G: int, H: int, W: int, scale: float, scratch=None, apod=None,
                grid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[G, M, 2] fp32 on the device: E x of the module docstring for img [H*W,2], maps [G*H*W,2] (device, fp32) at ``pos``
    [M, 2] (fp64, numpy or device tensor) -- inr_sense_nufft_prepare, torch.fft.fft2(ortho) of the plain-layout grid,
    inr_nufft_interp_plain, on the current stream.  ``grid`` [G,2H,2W,2], ``scratch``
    (trajectory.nufft_scratch_floats(G, H, W, M) floats), ``apod`` (trajectory.nufft_device_apodisation) and ``out`` are
    the caller's to reuse every step (defaults: made here)."""
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise RuntimeError("sense_nufft only runs on an MI355X (no CPU fallback; sense_nufft_numpy is the host-side "
                           "restatement)")
    p = T._device_positions(pos, img.device)
    ay_ax = _apod(apod, H, W, img.device)
    with torch.cuda.device(img.device):
        grid = sense_nufft_prepare(img, maps, G, H, W, scale, ay_ax, grid)
        k = torch.view_as_real(torch.fft.fft2(torch.view_as_complex(grid), norm="ortho"))
        return nufft_interp_plain(k, p, G, H, W, scratch, out)


def sense_nufft_adjoint(gk: torch.Tensor, maps: torch.Tensor, pos, shape, scale: float, weights=None,
                        dimg: Optional[torch.Tensor] = None, accumulate: bool = False, bins=None, apod=None, scratch=None,
                        grid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[H*W, 2] fp32 on the device: E^H (weights * gk) for gk [G, M, 2], maps [G*H*W,2] (device, fp32) --
    inr_nufft_spread_plain, torch.fft.ifft2(ortho), inr_sense_nufft_finish, on the current stream; ``shape`` = (H, W) or
    (G, H, W).  ``dimg`` is written, or added to with ``accumulate``.  ``bins``: trajectory.nufft_device_bins (default:
    made here, which reads device positions back); ``weights``: [M], used in fp32; the rest as for sense_nufft."""
    if not isinstance(gk, torch.Tensor) or not gk.is_cuda:
        raise RuntimeError("sense_nufft_adjoint only runs on an MI355X (no CPU fallback; sense_nufft_adjoint_numpy is the "
                           "host-side restatement)")
    G, M = int(gk.shape[0]), int(gk.shape[1])
    H, W = (int(v) for v in tuple(shape)[-2:])
    p = T._device_positions(pos, gk.device)
    if int(p.shape[0]) != M:
        raise ValueError(f"gk has {M} samples per coil, pos {int(p.shape[0])}")
    w = T._device_weights(weights, M, gk.device)
    bins = bins if bins is not None else T.nufft_device_bins(pos, H, W, gk.device)
    ay_ax = _apod(apod, H, W, gk.device)
    with torch.cuda.device(gk.device):
        grid = nufft_spread_plain(gk, p, w, bins, G, H, W, scratch, grid)
        g = torch.view_as_real(torch.fft.ifft2(torch.view_as_complex(grid), norm="ortho"))
        return sense_nufft_finish(g, maps, G, H, W, scale, ay_ax, dimg, accumulate)


class SenseNufft:
    """E and E^H for one set of maps and positions, with every buffer a step reuses made once: the device positions,
    the density weights in fp32, the spread's bins, the apodisation vectors, the taps' scratch and the grid."""

    def __init__(self, maps: torch.Tensor, pos, shape, scale: float, weights=None):
        self.G, self.H, self.W = (int(v) for v in shape[:3])
        dev = maps.device
        self.maps = maps.reshape(self.G * self.H * self.W, 2)
        self.scale = float(scale)
        self.pos = T._device_positions(pos, dev)
        self.M = int(self.pos.shape[0])
        self.weights = T._device_weights(weights, self.M, dev)
        self.bins = T.nufft_device_bins(pos, self.H, self.W, dev)
        self.apod = T.nufft_device_apodisation(self.H, self.W, dev)
        self.scratch = torch.empty(T.nufft_scratch_floats(self.G, self.H, self.W, self.M), device=dev)
        self.grid = torch.empty(self.G, 2 * self.H, 2 * self.W, 2, device=dev)

    def forward(self, img: torch.Tensor, scale: Optional[float] = None, out=None) -> torch.Tensor:
        return sense_nufft(img, self.maps, self.pos, self.G, self.H, self.W, self.scale if scale is None else scale,
                           self.scratch, self.apod, self.grid, out)

    def adjoint(self, gk: torch.Tensor, scale: Optional[float] = None, weighted: bool = False, dimg=None,
                accumulate: bool = False) -> torch.Tensor:
        return sense_nufft_adjoint(gk, self.maps, self.pos, (self.H, self.W), self.scale if scale is None else scale,
                                   self.weights if weighted else None, dimg, accumulate, self.bins, self.apod,
                                   self.scratch, self.grid)


@torch.no_grad()
def cg_sense_offgrid(op: SenseNufft, y: torch.Tensor, iters: int, lam: float = 0.0):
    """Non-Cartesian CG-SENSE on the device (cg_sense_nufft_numpy's iterations): E = op with scale 1, W = op.weights;
    y [G, M, 2].  The inner products are formed in fp64 on the device and read back.  Returns (iterates [H*W,2],
    objective)."""
    from .sense_calib import _cg_normal
    w64 = None if op.weights is None else op.weights.double()
    fwd = lambda x: op.forward(x.contiguous(), scale=1.0)
    adj = lambda k: op.adjoint(k.contiguous(), scale=1.0, weighted=True)
    dot = lambda u: float((u.double() ** 2).sum())

    def w_sum(a):
        e = (a.double() ** 2).sum(dim=-1)
        return float((e if w64 is None else e * w64[None, :]).sum())

    def normal(p):
        Ep = fwd(p)
        q = adj(Ep)
        return (q + lam * p if lam else q), w_sum(Ep) + lam * dot(p)

    def objective(x):
        return w_sum(y) if x is None else w_sum(fwd(x) - y) + lam * dot(x)

    axpy = lambda k, u, v: k * u if v is None else v + k * u
    return _cg_normal(adj(y), normal, dot, axpy, objective, int(iters))
