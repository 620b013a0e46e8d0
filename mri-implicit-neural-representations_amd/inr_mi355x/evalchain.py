"""Validation chain of train.py:199-242 on the device: no_grad forward sweep over all C*H*W
coordinates -> (C,H,W,2) -> centred orthonormal inverse FFT -> |.| -> root-sum-of-squares ->
PSNR (models/utils.py:236-250: max(x), not max(x)^2).  fastmri's ifft2c / complex_abs / rss are
third-party and absent offline; these follow their published definitions via torch.fft (hipFFT).
image_metrics / ssim run the RSS, PSNR and SSIM (models/utils.py:227-233, scikit-image 0.18.1) in the library's
kernels (inr_image_metrics); there is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L


def complex_abs(x: torch.Tensor) -> torch.Tensor:
    return (x ** 2).sum(dim=-1).sqrt()


def rss(x: torch.Tensor, dim: int = 0) -> torch.Tensor:
    return torch.sqrt((x ** 2).sum(dim))


def _fftc(x: torch.Tensor, inverse: bool) -> torch.Tensor:
    c = torch.view_as_complex(x.contiguous())
    c = torch.fft.ifftshift(c, dim=(-2, -1))
    c = (torch.fft.ifftn if inverse else torch.fft.fftn)(c, dim=(-2, -1), norm="ortho")
    c = torch.fft.fftshift(c, dim=(-2, -1))
    return torch.view_as_real(c)


def fft2c(x):
    return _fftc(x, False)


def ifft2c(x):
    return _fftc(x, True)


def psnr(x: torch.Tensor, xhat: torch.Tensor, epsilon: float = 1e-10) -> torch.Tensor:
    denom = torch.mean((x - xhat) ** 2)
    return 10 * torch.log10(torch.max(x) / (denom + epsilon))


def reconstruct(flat: torch.Tensor, shape, in_image_space: bool) -> torch.Tensor:
    C, H, W = shape
    im = flat.reshape(C, H, W, 2)
    if not in_image_space:
        im = ifft2c(im)
    return rss(complex_abs(im), dim=0)


def _dev_ptr(t: torch.Tensor, name: str, dtype) -> int:
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the image metrics only run on an MI355X (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    return t.data_ptr()


def metrics_scratch_doubles(C_: int, H: int, W: int) -> int:
    """fp64 words of scratch inr_image_metrics needs for [C,H,W,2] coil images."""
    n = C.c_int64()
    L.check(L.load().inr_image_metrics_scratch(C_, H, W, C.byref(n)))
    return int(n.value)


def image_metrics(ref_rss: Optional[torch.Tensor], coil_images: torch.Tensor, rss_out: Optional[torch.Tensor] = None,
                  metrics_out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """coil_images [C,H,W,2] fp32 (after ifft2c in k-space configs) -> (rss [H,W], metrics [8] fp64 on the device:
    psnr, ssim, sse, max_ref, min_ref, max_rec, min_rec, data_range), or (rss, None) when ref_rss is None.
    Buffers given by the caller are used as they are (no allocation inside: graph-capturable)."""
    if coil_images.dim() != 4 or coil_images.shape[-1] != 2:
        raise RuntimeError(f"coil_images has shape {tuple(coil_images.shape)}, expected [C,H,W,2]")
    C_, H, W = (int(v) for v in coil_images.shape[:3])
    dev = coil_images.device
    if rss_out is None:
        rss_out = torch.empty(H, W, device=dev, dtype=torch.float32)
    if tuple(rss_out.shape) != (H, W):
        raise RuntimeError(f"rss_out has shape {tuple(rss_out.shape)}, expected {(H, W)}")
    ref_p = mp = sp = None
    n_scratch = 0
    if ref_rss is not None:
        if tuple(ref_rss.shape) != (H, W):
            raise RuntimeError(f"ref_rss has shape {tuple(ref_rss.shape)}, expected {(H, W)}")
        ref_p = _dev_ptr(ref_rss, "ref_rss", torch.float32)
        if metrics_out is None:
            metrics_out = torch.empty(L.METRICS_WORDS, device=dev, dtype=torch.float64)
        if metrics_out.numel() < L.METRICS_WORDS:
            raise RuntimeError(f"metrics_out holds {metrics_out.numel()} doubles, needs {L.METRICS_WORDS}")
        if scratch is None:
            scratch = torch.empty(max(1, metrics_scratch_doubles(C_, H, W)), device=dev, dtype=torch.float64)
        mp = _dev_ptr(metrics_out, "metrics_out", torch.float64)
        sp = _dev_ptr(scratch, "scratch", torch.float64)
        n_scratch = scratch.numel()
    lib = L.load()
    L.check(lib.inr_image_metrics(_dev_ptr(coil_images, "coil_images", torch.float32), C_, H, W, ref_p,
                                  _dev_ptr(rss_out, "rss_out", torch.float32), mp, sp, n_scratch,
                                  torch.cuda.current_stream(dev).cuda_stream))
    return rss_out, (metrics_out if ref_rss is not None else None)


def ssim(x: torch.Tensor, xhat: torch.Tensor) -> torch.Tensor:
    """models/utils.py:227-233 on device images [H,W] fp32: structural_similarity(x, xhat, data_range=R) of
    scikit-image 0.18.1, R = max(x.max, xhat.max) - min(x.min, xhat.min).  Returns a fp64 device scalar.
    xhat enters as the magnitude of a one-coil image: it must be non-negative, as RSS images are."""
    if xhat.dim() != 2:
        raise RuntimeError(f"xhat has shape {tuple(xhat.shape)}, expected [H,W]")
    # one coil whose |z| is xhat: the RSS pass reproduces it exactly (sqrt(x^2) = |x| for x >= 0; sign is lost otherwise)
    if not xhat.is_cuda:
        raise RuntimeError(f"xhat is on {xhat.device}: the image metrics only run on an MI355X (no CPU fallback)")
    coil = torch.stack((xhat, torch.zeros_like(xhat)), dim=-1).unsqueeze(0).contiguous()
    return image_metrics(x.contiguous(), coil)[1][1]
