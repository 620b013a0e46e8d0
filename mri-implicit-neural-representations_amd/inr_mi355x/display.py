"""The pictures and the per-coil table of the validation epoch (train.py:136-143,221-238; models/utils.py:35-44,254-287)
without matplotlib / PIL at run time: display scaling, 8-bit quantisation and coil statistics are the library's kernels
(inr_kspace_display, inr_gray8, inr_coil_stats; there is no CPU path), the host only receives H*W bytes per picture and
4*C doubles and writes 8-bit greyscale PNG files with zlib + struct."""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from typing import Optional

import numpy as np
import torch

from . import _lib as L

STATS_TITLE = "K-space Reconstruction Statistics Per Coil"  # models/utils.py:286 (the reference hard-codes "K-space")
STATS_HEADERS = ["coil", "mean", "std", "max", "min"]


def gray_lut() -> np.ndarray:
    """The 256 bytes matplotlib's 'gray' map hands to a PNG: its table is linspace(0, 1, 256) = i * (1 / 255) in float64,
    and to_rgba(bytes=True) stores uint8(trunc(table * 255)).  Not the identity: i - 1 at i = 33, 37, 41, 45, ...
    (tests/golden/display.npz holds the table matplotlib 3.10 produced)."""
    step = 1.0 / 255.0
    return np.array([int(i * step * 255.0) for i in range(256)], dtype=np.uint8)


_LUT_DEV = {}


def _device_lut(dev: torch.device) -> torch.Tensor:
    """The table on `dev`, uploaded once."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _LUT_DEV:
        _LUT_DEV[key] = torch.from_numpy(gray_lut()).to(dev)
    return _LUT_DEV[key]


def _dev_ptr(t: torch.Tensor, name: str, dtype) -> int:
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the display kernels only run on an MI355X (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    return t.data_ptr()


def _coil_shape(coils: torch.Tensor, name: str = "coils"):
    if coils.dim() != 4 or coils.shape[-1] != 2:
        raise RuntimeError(f"{name} has shape {tuple(coils.shape)}, expected [C,H,W,2]")
    return tuple(int(v) for v in coils.shape[:3])


def _out(buf: Optional[torch.Tensor], shape, dev, dtype, name: str) -> torch.Tensor:
    if buf is None:
        return torch.empty(*shape, device=dev, dtype=dtype)
    if tuple(buf.shape) != tuple(shape):
        raise RuntimeError(f"{name} has shape {tuple(buf.shape)}, expected {tuple(shape)}")
    return buf


def kspace_display_scratch_floats(C_: int, H: int, W: int) -> int:
    n = C.c_int64()
    L.check(L.load().inr_kspace_display_scratch(C_, H, W, C.byref(n)))
    return int(n.value)


def gray8_scratch_floats(H: int, W: int) -> int:
    n = C.c_int64()
    L.check(L.load().inr_gray8_scratch(H, W, C.byref(n)))
    return int(n.value)


def coil_stats_scratch_doubles(C_: int, H: int, W: int) -> int:
    n = C.c_int64()
    L.check(L.load().inr_coil_stats_scratch(C_, H, W, C.byref(n)))
    return int(n.value)


def kspace_display(coils: torch.Tensor, minus: Optional[torch.Tensor] = None, smoothing_factor: float = 8.0,
                   out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """save_im's is_kspace branch (models/utils.py:262-267): coils [C,H,W,2] fp32 (minus `minus`, when given: the error
    picture) -> [H,W] fp32 in 0..1 = log1p(rss * expm1(sf) / max) / max.  An all-zero input gives NaN, as the
    reference's 0 / 0.  Buffers given by the caller are used as they are (no allocation inside: graph-capturable)."""
    C_, H, W = _coil_shape(coils)
    if minus is not None and tuple(minus.shape) != tuple(coils.shape):
        raise RuntimeError(f"minus has shape {tuple(minus.shape)}, expected {tuple(coils.shape)}")
    cp = _dev_ptr(coils, "coils", torch.float32)
    mp = None if minus is None else _dev_ptr(minus, "minus", torch.float32)
    dev = coils.device
    out = _out(out, (H, W), dev, torch.float32, "out")
    if scratch is None:
        scratch = torch.empty(kspace_display_scratch_floats(C_, H, W), device=dev, dtype=torch.float32)
    L.check(L.load().inr_kspace_display(cp, mp, C_, H, W, float(smoothing_factor), _dev_ptr(out, "out", torch.float32),
                                        _dev_ptr(scratch, "scratch", torch.float32), scratch.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream))
    return out


def gray8(img: torch.Tensor, take_abs: bool = False, vmin: Optional[float] = None, vmax: Optional[float] = None,
          out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None,
          norm_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img [H,W] fp32 -> [H,W] uint8: the R channel plt.imsave(..., cmap="gray") writes.  vmin / vmax follow save_im's
    ``if vmin and vmax`` (models/utils.py:256): a missing or zero bound means the picture's own extrema.  norm_out
    (optional, [H,W] fp32) receives the normalised value before quantisation."""
    if img.dim() != 2:
        raise RuntimeError(f"img has shape {tuple(img.shape)}, expected [H,W]")
    H, W = (int(v) for v in img.shape)
    ip = _dev_ptr(img, "img", torch.float32)
    dev = img.device
    out = _out(out, (H, W), dev, torch.uint8, "out")
    has_range = bool(vmin and vmax)
    sp, ns = None, 0
    if not has_range:
        if scratch is None:
            scratch = torch.empty(gray8_scratch_floats(H, W), device=dev, dtype=torch.float32)
        sp, ns = _dev_ptr(scratch, "scratch", torch.float32), scratch.numel()
    npp = None
    if norm_out is not None:
        if tuple(norm_out.shape) != (H, W):
            raise RuntimeError(f"norm_out has shape {tuple(norm_out.shape)}, expected {(H, W)}")
        npp = _dev_ptr(norm_out, "norm_out", torch.float32)
    L.check(L.load().inr_gray8(ip, H, W, int(bool(take_abs)), int(has_range), float(vmin) if has_range else 0.0,
                               float(vmax) if has_range else 0.0, _device_lut(dev).data_ptr(),
                               _dev_ptr(out, "out", torch.uint8), npp, sp, ns, torch.cuda.current_stream(dev).cuda_stream))
    return out


def coil_stats(coils: torch.Tensor, stats: Optional[torch.Tensor] = None,
               scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stats_per_coil's numbers (models/utils.py:274-283): coils [C,H,W,2] fp32 -> [C,4] fp64 on the device = mean,
    unbiased std, max, min of each coil's 2*H*W values, accumulated in fp64."""
    C_, H, W = _coil_shape(coils)
    cp = _dev_ptr(coils, "coils", torch.float32)
    dev = coils.device
    stats = _out(stats, (C_, 4), dev, torch.float64, "stats")
    if scratch is None:
        scratch = torch.empty(coil_stats_scratch_doubles(C_, H, W), device=dev, dtype=torch.float64)
    L.check(L.load().inr_coil_stats(cp, C_, H, W, _dev_ptr(stats, "stats", torch.float64),
                                    _dev_ptr(scratch, "scratch", torch.float64), scratch.numel(),
                                    torch.cuda.current_stream(dev).cuda_stream))
    return stats


# ---- host side: PNG files, the table, the folder tree ------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _as_u8(u8) -> np.ndarray:
    a = u8.detach().cpu().numpy() if isinstance(u8, torch.Tensor) else np.asarray(u8)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"an 8-bit greyscale picture is a non-empty [H,W] uint8 array (got {a.dtype} {a.shape})")
    return a


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png_gray(path: str, u8, level: int = 6) -> None:
    """[H,W] uint8 (tensor or array) -> an 8-bit greyscale PNG (colour type 0, filter 0 on every row)."""
    a = _as_u8(u8)
    H, W = a.shape
    rows = np.zeros((H, W + 1), dtype=np.uint8)  # a filter-type byte in front of every scanline
    rows[:, 1:] = a
    png = (_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


def read_png_gray(path: str) -> np.ndarray:
    """An 8-bit greyscale, non-interlaced PNG -> [H,W] uint8 (all five scanline filters)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: bad CRC in chunk {tag!r}")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None or hdr[2:] != (8, 0, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit greyscale, non-interlaced PNG files are read here (IHDR {hdr})")
    W, H = hdr[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8).reshape(H, W + 1)
    out = np.zeros((H, W), dtype=np.uint8)
    prev = np.zeros(W, dtype=np.int64)
    for y in range(H):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:  # 1 (sub), 3 (average), 4 (Paeth): each byte needs its left neighbour
            cur = np.zeros(W, dtype=np.int64)
            for x in range(W):
                a = cur[x - 1] if x else 0
                b, c = prev[x], (prev[x - 1] if x else 0)
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) // 2
                elif ft == 4:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                else:
                    raise ValueError(f"{path}: filter type {ft}")
                cur[x] = (line[x] + pred) & 255
        out[y] = cur
        prev = cur
    return out


def coil_stats_table(stats) -> str:
    """The text stats_per_coil prints (models/utils.py:284-287): title line, then tabulate's table of
    (coil, mean, std, max, min); a fixed-width table of the same numbers when tabulate is not installed."""
    rows = [(i, *(float(v) for v in r)) for i, r in enumerate(np.asarray(
        stats.detach().cpu() if isinstance(stats, torch.Tensor) else stats, dtype=np.float64).reshape(-1, 4))]
    try:
        from tabulate import tabulate
        table = tabulate(rows, headers=STATS_HEADERS)
    except ImportError:
        cells = [STATS_HEADERS] + [[str(r[0])] + ["%.6g" % v for v in r[1:]] for r in rows]
        widths = [max(len(c[k]) for c in cells) + (2 if k else 0) for k in range(5)]
        lines = ["".join(c[k].rjust(widths[k]) for k in range(5)) for c in cells]
        lines.insert(1, "".join(("-" * (widths[k] - (2 if k else 0))).rjust(widths[k]) for k in range(5)))
        table = "\n".join(lines)
    return "{}\n{}".format(STATS_TITLE, table)


def prepare_sub_folder(output_directory: str):
    """models/utils.py:35-44: <output>/images and <output>/checkpoints, created when missing -> (checkpoints, images)."""
    image_directory = os.path.join(output_directory, "images")
    checkpoint_directory = os.path.join(output_directory, "checkpoints")
    for d in (image_directory, checkpoint_directory):
        if not os.path.exists(d):
            print("Creating directory: {}".format(d))
            os.makedirs(d)
    return checkpoint_directory, image_directory
