"""SENSE-model fits (no reference counterpart): the one piece of MRI physics the per-coil fits do
not have -- all coils show the same anatomy through different smooth sensitivity maps.  Two coordinate networks in
IMAGE space, fitted to k-space data:

    X_g[y,x] = scale * S_g[y,x] * I[y,x]        (complex product; a (re, im) pair is one complex number)
    K_g      = fft2c(X_g)                        (evalchain.fft2c: centred, orthonormal)
    loss     = the pointwise loss of inr_loss_grad on (K, gt, mask), inv_count = 1 / sampled rows of the group

and back through the adjoint chain: gK = dloss/dK, gX = ifft2c(gK) (the orthonormal transform is unitary: its adjoint is
its inverse), dS_g = scale * conj(I) * gX_g, dI = scale * sum_g conj(S_g) * gX_g.

Here: the permutation the kernels and the trainer's ingest share (``shift_index``), the fp32 numpy text of the two
kernels of csrc/inr_sense.hip, bit for bit (``sense_apply_numpy``, ``sense_grad_numpy``), the float64 statement of the
whole chain (``sense_chain_numpy``, the oracle of tests/test_sense_host.py and tests/test_gpu_sense.py), and the ctypes
bindings on device tensors.  inr_mi355x/train_sense.py drives the two engines; inr_mi355x/reconstruct.py renders their
checkpoints.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import LossSpec, _ptr, _same_device, _shape


IMAGE_PREFIX, SENS_PREFIX = "image.", "sens."


# ---- checkpoint keys (train_sense.py writes them, reconstruct.py reads them) -------------------------------------------
def has_sense_keys(net_state: dict) -> bool:
    return any(k.startswith((IMAGE_PREFIX, SENS_PREFIX)) for k in net_state)


def join_state(image_state: dict, sens_state: dict) -> OrderedDict:
    """'image.' + the image network's keys, then 'sens.' + the sensitivity network's (clones: a checkpoint must not alias
    the running weights).  Kept for callers outside the package: the trainer writes the same keys through
    checkpoint.joined_net over its _parts()."""
    return OrderedDict((prefix + k, v.detach().clone()) for prefix, sd in ((IMAGE_PREFIX, image_state),
                                                                          (SENS_PREFIX, sens_state))
                       for k, v in sd.items())


def split_state(net_state: dict):
    """(image network state_dict, sensitivity network state_dict) of join_state's"""
    from .checkpoint import split_prefixed
    img, sen = split_prefixed(net_state, (IMAGE_PREFIX, SENS_PREFIX))
    if not img or not sen:
        raise ValueError(f"a SENSE checkpoint holds both '{IMAGE_PREFIX}' and '{SENS_PREFIX}' keys")
    return img, sen


def sens_encoder_config(settings: dict, encoder_config: dict) -> dict:
    """the sensitivity network's encoder: the main one with settings['encoder']'s scale and embedding_size"""
    return dict(encoder_config, scale=settings["encoder"]["scale"], embedding_size=settings["encoder"]["embedding_size"])


# ---- the shift -----------------------------------------------------------------------------------------------------------
def place_index(H: int, W: int) -> np.ndarray:
    """int64 [H*W]: q of every pixel p = y*W + x -- where the kernels put it under shift = 1,
    q = ((y - H//2) mod H) * W + (x - W//2) mod W."""
    y, x = np.divmod(np.arange(H * W, dtype=np.int64), W)
    return ((y - H // 2) % H) * W + (x - W // 2) % W


def shift_index(H: int, W: int) -> np.ndarray:
    """int64 [H*W]: the permutation of a plane under torch.fft.ifftshift over (H, W), for every parity of H and W:
    ``plane.reshape(-1)[shift_index(H, W)]`` is ``ifftshift(plane).reshape(-1)``.  The inverse of place_index: entry q
    names the pixel the kernels store at q.  The trainer's ingest shifts targets and mask with it once."""
    perm = np.empty(H * W, dtype=np.int64)
    perm[place_index(H, W)] = np.arange(H * W, dtype=np.int64)
    return perm


# ---- the two kernels in fp32 numpy -------------------------------------------------------------------------------------
def _f32(a, *shape) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(*shape)


def sense_apply_numpy(img, sens, G: int, H: int, W: int, scale: float, shift: int) -> np.ndarray:
    """x [G,H,W,2] fp32: the text of inr_sense_apply -- every product and sum one fp32 operation, in the kernel's order."""
    img, sens, s = _f32(img, H * W, 2), _f32(sens, G, H * W, 2), np.float32(scale)
    ir, ii = img[None, :, 0], img[None, :, 1]
    sr, si = sens[..., 0], sens[..., 1]
    re = sr * ir - si * ii
    im = sr * ii + si * ir
    out = np.stack((s * re, s * im), axis=-1)
    x = np.empty_like(out)
    x[:, place_index(H, W) if shift else np.arange(H * W)] = out
    return x.reshape(G, H, W, 2)


def sense_grad_numpy(img, sens, gx, G: int, H: int, W: int, scale: float, shift: int) -> Tuple[np.ndarray, np.ndarray]:
    """(dimg [H*W,2], dsens [G*H*W,2]) fp32: the text of inr_sense_grad; dimg is summed from zero in coil order."""
    img, sens, s = _f32(img, H * W, 2), _f32(sens, G, H * W, 2), np.float32(scale)
    g = _f32(gx, G, H * W, 2)[:, place_index(H, W) if shift else np.arange(H * W)]
    ir, ii = img[:, 0], img[:, 1]
    dimg = np.zeros((H * W, 2), dtype=np.float32)
    dsens = np.empty((G, H * W, 2), dtype=np.float32)
    for k in range(G):
        ur, ui = s * g[k, :, 0], s * g[k, :, 1]
        sr, si = sens[k, :, 0], sens[k, :, 1]
        dsens[k, :, 0] = ir * ur + ii * ui
        dsens[k, :, 1] = ir * ui - ii * ur
        dimg[:, 0] = dimg[:, 0] + (sr * ur + si * ui)
        dimg[:, 1] = dimg[:, 1] + (sr * ui - si * ur)
    return dimg, dsens.reshape(G * H * W, 2)


# ---- the whole chain in float64 ----------------------------------------------------------------------------------------
def _c(a: np.ndarray) -> np.ndarray:
    return a[..., 0] + 1j * a[..., 1]


def _pairs(z: np.ndarray) -> np.ndarray:
    return np.stack((z.real, z.imag), axis=-1)


def fft2c_numpy(x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """evalchain.fft2c / ifft2c over the last two axes of a complex array, in float64"""
    f = np.fft.ifft2 if inverse else np.fft.fft2
    return np.fft.fftshift(f(np.fft.ifftshift(x, axes=(-2, -1)), axes=(-2, -1), norm="ortho"), axes=(-2, -1))


def sense_chain_numpy(img, sens, gt, mask, loss: LossSpec, count: int, G: int, H: int, W: int, scale: float,
                      hdr_A: float = 0.0, parts: bool = False):
    """(loss, dimg [H*W,2], dsens [G*H*W,2]) in float64 for img [H*W,2], sens [G*H*W,2], gt [G*H*W,2] and mask [G*H*W]
    (or None) in the DATASET's own order (nothing shifted): the module docstring's chain with np.fft and the pointwise
    loss rows of gain.loss_rows_float64.  ``count`` = rows entering the mean (the sampled rows of the group).
    ``parts``: also the two arrays between the kernels and the transforms, X and gX [G,H,W,2]."""
    from .gain import loss_rows_float64
    I = _c(np.asarray(img, dtype=np.float64).reshape(H, W, 2))
    S = _c(np.asarray(sens, dtype=np.float64).reshape(G, H, W, 2))
    gt = np.asarray(gt, dtype=np.float64).reshape(G * H * W, 2)
    keep = np.ones(G * H * W, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    X = scale * S * I[None]
    K = _pairs(fft2c_numpy(X)).reshape(G * H * W, 2)
    gK = np.zeros_like(K)
    total = 0.0
    if keep.any():
        Lr, g = loss_rows_float64(loss, K[keep], gt[keep], 1.0 / float(count), hdr_A)
        total = float(np.sum(Lr))
        gK[keep] = g
    gX = fft2c_numpy(_c(gK.reshape(G, H, W, 2)), inverse=True)
    dS = scale * np.conj(I)[None] * gX
    dI = scale * np.sum(np.conj(S) * gX, axis=0)
    out = (total, _pairs(dI).reshape(H * W, 2), _pairs(dS).reshape(G * H * W, 2))
    return out + (_pairs(X), _pairs(gX)) if parts else out


# ---- the kernels -------------------------------------------------------------------------------------------------------
def sense_apply(img: torch.Tensor, sens: torch.Tensor, G: int, H: int, W: int, scale: float, shift: int = 1,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inr_sense_apply on device tensors img [H*W,2], sens [G*H*W,2] -> x [G,H,W,2] (``out`` when given): the coil images
    scale * S_g * I, stored where ifftshift puts them when ``shift``."""
    _shape(img, "img", H * W, 2)
    _shape(sens, "sens", G * H * W, 2)
    x = torch.empty(G, H, W, 2, device=img.device) if out is None else out
    _shape(x, "out", G, H, W, 2)
    pi, ps, px = _ptr(img, "img"), _ptr(sens, "sens"), _ptr(x, "out")
    _same_device(img, sens=sens, out=x)
    L.launch("inr_sense_apply", img.device, pi, ps, G, H, W, float(scale), int(shift), px)
    return x


def sense_grad(img: torch.Tensor, sens: torch.Tensor, gx: torch.Tensor, G: int, H: int, W: int, scale: float,
               shift: int = 1, dimg: Optional[torch.Tensor] = None, dsens: Optional[torch.Tensor] = None):
    """inr_sense_grad on device tensors img [H*W,2], sens [G*H*W,2], gx [G,H,W,2] -> (dimg [H*W,2], dsens [G*H*W,2])"""
    _shape(img, "img", H * W, 2)
    _shape(sens, "sens", G * H * W, 2)
    _shape(gx, "gx", G, H, W, 2)
    dimg = torch.empty_like(img) if dimg is None else dimg
    dsens = torch.empty_like(sens) if dsens is None else dsens
    _shape(dimg, "dimg", H * W, 2)
    _shape(dsens, "dsens", G * H * W, 2)
    ptrs = (_ptr(img, "img"), _ptr(sens, "sens"), _ptr(gx, "gx"), _ptr(dimg, "dimg"), _ptr(dsens, "dsens"))
    _same_device(img, sens=sens, gx=gx, dimg=dimg, dsens=dsens)
    L.launch("inr_sense_grad", img.device, ptrs[0], ptrs[1], ptrs[2], G, H, W, float(scale), int(shift), ptrs[3], ptrs[4])
    return dimg, dsens
