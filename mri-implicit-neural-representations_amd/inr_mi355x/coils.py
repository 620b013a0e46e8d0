"""Software coil compression (inr_coil_gram / inr_coil_apply, csrc/inr_coils.hip; Huang et al. 2008): fit
K virtual coils, the principal components of the coil covariance, instead of the C physical ones.  The reference has no
counterpart; the switch is config['virtual_coils'] (absent or 0: off, and then nothing here runs).

Data are ``x[c][p]``: complex, fp32 (re, im) pairs, coil-major [C, N, 2] with N = H*W -- the resident layout of datasets.py.

    Gram matrix         G[i][j] = sum_p x_i[p] conj(x_j[p]); C x C complex fp64, both triangles.  Every product is formed
                        in fp64 from the fp32 inputs, every sum is fp64.
    compression matrix  numpy.linalg.eigh(G) in float64 on the host.  A is K x C: its rows are the conjugated
                        eigenvectors of the K largest eigenvalues, in descending order, each multiplied by a unit complex
                        number so that its entry of largest modulus (the first such on ties) is real and positive; cast
                        to complex64 for use.  energy_kept = sum of the K largest eigenvalues / trace(G).
    apply               y_m[p] = sum_k A[m][k] x_k[p] in fp32, k = 0..C-1 in order (re += ar xr - ai xi,
                        im += ar xi + ai xr).  Compression uses A, expansion back to physical coils its conjugate
                        transpose, through the same entry point.
    compression loss    rss_psnr = evalchain.psnr(rss of the physical coils, rss of the virtual coils), on the data before
                        normalisation; in k-space mode both RSS images come from evalchain.ifft2c.

``coil_gram_numpy``, ``compression_matrix`` and ``coil_apply_numpy`` are these definitions in numpy and need no GPU; the
kernels differ from them only in the order of the fp64 sums (Gram) and in fp32 rounding (apply).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L


def _as_complex(x) -> np.ndarray:
    """[..., 2] float pairs (array or CPU tensor) or a complex array -> complex ndarray of the same precision"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return x
    if x.shape[-1] != 2:
        raise ValueError(f"expected (re, im) pairs in the last axis, got shape {x.shape}")
    x = np.ascontiguousarray(x)
    return x.view(np.complex64 if x.dtype == np.float32 else np.complex128)[..., 0]


def _pairs(z: np.ndarray, dtype) -> np.ndarray:
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1), dtype=dtype)  # row-major whatever z's strides


def check_virtual_coils(value, coils: Optional[int] = None) -> int:
    """config['virtual_coils'] -> K (0: off).  ValueError for a non-integer, K < 0, K > ``coils`` or, with the switch on,
    ``coils`` > INR_COIL_MAX."""
    if value is None:
        return 0
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"virtual_coils = {value!r}: an integer number of virtual coils (0 or absent: off)")
    K = int(value)
    if K < 0:
        raise ValueError(f"virtual_coils = {K}: must be >= 0")
    if K and coils is not None:
        if coils > L.COIL_MAX:
            raise ValueError(f"virtual_coils with {coils} physical coils: coil compression takes at most {L.COIL_MAX}")
        if K > coils:
            raise ValueError(f"virtual_coils = {K} > the scan's {coils} coils")
    return K


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def coil_gram_numpy(data, shape=None) -> np.ndarray:
    """[C, C] complex128.  ``data``: [C, ..., 2] pairs or a complex [C, ...] array (``shape`` = (C, ...) for flat rows)."""
    z = _as_complex(data)
    z = z.reshape(int(shape[0]), -1) if shape is not None else z.reshape(z.shape[0], -1)
    if z.dtype != np.complex64:
        raise ValueError("the Gram matrix is defined on fp32 data")
    z64 = z.astype(np.complex128)
    zc = z64.conj()
    G = np.empty((z.shape[0], z.shape[0]), dtype=np.complex128)
    for i in range(z.shape[0]):
        G[i] = (z64[i][None, :] * zc).sum(axis=1)  # exact products, fp64 sums
    return G


def compression_matrix(G, K, dtype=np.complex64) -> Tuple[np.ndarray, np.ndarray, float]:
    """(A [K, C] complex64, eigenvalues [C] fp64 in descending order, energy_kept) of a Gram matrix.  ``dtype``:
    numpy.complex128 gives A before its cast (orthonormal rows to rounding of float64)."""
    G = np.asarray(G)
    if not np.iscomplexobj(G):
        G = _as_complex(G)
    G = G.astype(np.complex128)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f"G must be C x C, got {G.shape}")
    Cn = G.shape[0]
    K = check_virtual_coils(K, Cn)
    if K < 1:
        raise ValueError("compression_matrix needs K >= 1")
    w, V = np.linalg.eigh(G)  # ascending
    order = np.arange(Cn)[::-1]
    w, V = w[order], V[:, order]
    A = V[:, :K].conj().T.copy()
    for m in range(K):
        k = int(np.argmax(np.abs(A[m])))  # the first on ties
        A[m] *= np.conj(A[m, k]) / np.abs(A[m, k])
        A[m, k] = np.abs(A[m, k])  # exactly real
    return A.astype(dtype), w, float(w[:K].sum() / np.trace(G).real)


def coil_apply_numpy(A, x, shape=None) -> np.ndarray:
    """[M, N] complex64 = A [M, K] times x [K, N], fp32 throughout, k in order."""
    A = np.asarray(_as_complex(A)).astype(np.complex64)
    z = _as_complex(x)
    z = z.reshape(int(shape[0]), -1) if shape is not None else z.reshape(z.shape[0], -1)
    if z.dtype != np.complex64:
        raise ValueError("apply is defined on fp32 data")
    M, K = A.shape
    if K != z.shape[0]:
        raise ValueError(f"A is {A.shape}, the data has {z.shape[0]} coils")
    yr = np.zeros((M, z.shape[1]), dtype=np.float32)
    yi = np.zeros((M, z.shape[1]), dtype=np.float32)
    xr, xi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    for m in range(M):
        for k in range(K):
            ar, ai = np.float32(A[m, k].real), np.float32(A[m, k].imag)
            yr[m] += ar * xr[k] - ai * xi[k]
            yi[m] += ar * xi[k] + ai * xr[k]
    return (yr + 1j * yi).astype(np.complex64)


# ---- the kernels -------------------------------------------------------------------------------------------------------
_scratch = {}  # (C, N, device) -> (gram [C,C,2] fp64, scratch fp64)


def scratch_doubles(coils: int, n: int) -> int:
    out = C.c_int64(0)
    L.check(L.load().inr_coil_gram_scratch(int(coils), int(n), C.byref(out)))
    return int(out.value)


def _device_rows(t, name: str, coils: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: coil compression only runs on an MI355X (no CPU fallback; coil_gram_numpy / "
                           "coil_apply_numpy are the host-side definitions)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (re, im) pairs (got {t.dtype})")
    t = t.reshape(coils, -1, 2)
    return t if t.is_contiguous() else t.contiguous()


def coil_gram_device(data: torch.Tensor, shape) -> torch.Tensor:
    """One inr_coil_gram call on the current stream -> [C, C, 2] fp64 DEVICE tensor, valid until the next call with the
    same (C, N, device).  Nothing is read back."""
    coils = int(shape[0])
    check_virtual_coils(1, coils)
    x = _device_rows(data, "data", coils)
    n = x.shape[1]
    if n < 1:
        raise ValueError("coil_gram of no pixels")
    key = (coils, n, x.device)
    if key not in _scratch:
        _scratch[key] = (torch.empty(coils, coils, 2, device=x.device, dtype=torch.float64),
                         torch.empty(scratch_doubles(coils, n), device=x.device, dtype=torch.float64))
    gram, scratch = _scratch[key]
    L.launch("inr_coil_gram", x.device, x.data_ptr(), coils, n, gram.data_ptr(), scratch.data_ptr(), scratch.numel())
    return gram


def coil_gram(data: torch.Tensor, shape) -> np.ndarray:
    """Device tensor [(C*N), 2] / [C, ..., 2] with ``shape`` = (C, ...) -> [C, C] complex128 on the host."""
    return _as_complex(coil_gram_device(data, shape).cpu().numpy())


def coil_apply(data: torch.Tensor, A, shape) -> torch.Tensor:
    """[M, N, 2] fp32 on the device: A [M, K] (complex array, or [M, K, 2] pairs) times the K coil rows of ``data``
    (``shape`` = (K, ...))."""
    coils = int(shape[0])
    x = _device_rows(data, "data", coils)
    if isinstance(A, torch.Tensor):
        A = A.detach().cpu().numpy()
    Ac = np.asarray(_as_complex(A)).astype(np.complex64)
    if Ac.ndim != 2 or Ac.shape[1] != coils:
        raise ValueError(f"A is {Ac.shape}, the data has {coils} coils")
    M = int(Ac.shape[0])
    if not (1 <= M <= L.COIL_MAX and 1 <= coils <= L.COIL_MAX):
        raise ValueError(f"A is {Ac.shape}: at most {L.COIL_MAX} coils on either side")
    n = x.shape[1]
    if n < 1:
        raise ValueError("coil_apply of no pixels")
    a_dev = torch.from_numpy(_pairs(Ac, np.float32)).to(x.device).contiguous()  # [M, K, 2] row-major
    out = torch.empty(M, n, 2, device=x.device, dtype=torch.float32)
    L.launch("inr_coil_apply", x.device, x.data_ptr(), a_dev.data_ptr(), M, coils, n, out.data_ptr())
    return out


# ---- the record --------------------------------------------------------------------------------------------------------
@dataclass
class CoilCompression:
    matrix: np.ndarray  # [K, C] complex64
    eigenvalues: np.ndarray  # [C] fp64, descending
    coils_in: int
    coils_out: int
    energy_kept: float
    rss_psnr: Optional[float] = None

    def summary(self) -> dict:
        """what the JSON result and the validation records carry"""
        return {"coils_in": self.coils_in, "coils_out": self.coils_out, "energy_kept": self.energy_kept,
                "rss_psnr": self.rss_psnr}

    def state(self) -> dict:
        """the checkpoint's 'coil_compression' entry"""
        return {"matrix": torch.from_numpy(self.matrix.copy()), "eigenvalues": torch.from_numpy(self.eigenvalues.copy()),
                "coils_in": self.coils_in, "coils_out": self.coils_out, "energy_kept": self.energy_kept,
                "rss_psnr": self.rss_psnr}

    @classmethod
    def from_state(cls, st: dict) -> "CoilCompression":
        to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return cls(to_np(st["matrix"]).astype(np.complex64), to_np(st["eigenvalues"]).astype(np.float64),
                   int(st["coils_in"]), int(st["coils_out"]), float(st["energy_kept"]), st.get("rss_psnr"))

    def apply(self, physical: torch.Tensor) -> torch.Tensor:
        """physical [C, H, W, 2] (or [(C*H*W), 2]) on the device -> virtual [K, ..., 2] with this record's matrix"""
        out = coil_apply(physical, self.matrix, (self.coils_in,))
        return out.reshape(self.coils_out, *physical.shape[1:]) if physical.dim() == 4 else out

    def expand(self, virtual: torch.Tensor) -> torch.Tensor:
        """virtual [K, H, W, 2] on the device -> physical [C, H, W, 2]: the projection of the scan on the K components"""
        out = coil_apply(virtual, self.matrix.conj().T, (self.coils_out,))
        return out.reshape(self.coils_in, *virtual.shape[1:]) if virtual.dim() == 4 else out

    def expand_numpy(self, virtual) -> np.ndarray:
        return coil_apply_numpy(self.matrix.conj().T, virtual, (self.coils_out,))


def same_compression(a: Optional[dict], b: Optional[dict]) -> Optional[str]:
    """None when two checkpoint entries (or absences) describe the same compression, else what differs"""
    if (a is None) != (b is None):
        return "one side has coil compression and the other has none"
    if a is not None and (int(a["coils_in"]), int(a["coils_out"])) != (int(b["coils_in"]), int(b["coils_out"])):
        return (f"coil compression {int(a['coils_in'])} -> {int(a['coils_out'])} against "
                f"{int(b['coils_in'])} -> {int(b['coils_out'])}")
    return None


def _rss_psnr(physical: torch.Tensor, virtual: torch.Tensor, in_image_space: bool) -> float:
    from .evalchain import psnr, reconstruct
    ref = reconstruct(physical, physical.shape[:3], in_image_space)
    return float(psnr(ref, reconstruct(virtual, virtual.shape[:3], in_image_space)))


def compress(data: torch.Tensor, K, in_image_space: bool = False) -> Tuple[torch.Tensor, CoilCompression]:
    """data [C, H, W, 2] fp32 on the device, before normalisation -> (virtual [K, H, W, 2], CoilCompression): the Gram
    kernel, eigh on the host, the apply kernel, and rss_psnr of the result (``in_image_space``: the data are coil images,
    else k-space)."""
    if data.dim() != 4 or data.shape[-1] != 2:
        raise ValueError(f"compress takes [C, H, W, 2], got {tuple(data.shape)}")
    coils = int(data.shape[0])
    K = check_virtual_coils(K, coils)
    if K < 1:
        raise ValueError("compress needs K >= 1")
    G = coil_gram(data, (coils,))
    A, w, kept = compression_matrix(G, K)
    rec = CoilCompression(A, w, coils, K, kept)
    virtual = rec.apply(data.contiguous())
    rec.rss_psnr = _rss_psnr(data, virtual, in_image_space)
    return virtual, rec


def compress_numpy(data, K, in_image_space: bool = False) -> Tuple[np.ndarray, CoilCompression]:
    """compress() from the numpy definitions alone (CPU): [C, H, W, 2] pairs -> ([K, H, W, 2] fp32, CoilCompression)"""
    x = data.detach().cpu().numpy() if isinstance(data, torch.Tensor) else np.asarray(data)
    coils = int(x.shape[0])
    K = check_virtual_coils(K, coils)
    if K < 1:
        raise ValueError("compress needs K >= 1")
    A, w, kept = compression_matrix(coil_gram_numpy(x), K)
    rec = CoilCompression(A, w, coils, K, kept)
    virtual = _pairs(coil_apply_numpy(A, x), np.float32).reshape(K, *x.shape[1:])
    rec.rss_psnr = _rss_psnr(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), torch.from_numpy(virtual),
                             in_image_space)
    return virtual, rec


def add_virtual_coils_flag(ap) -> None:
    ap.add_argument("--virtual-coils", type=int, default=None, metavar="K",
                    help="fit K virtual coils, the principal components of the coil covariance, instead of the scan's "
                         "physical coils (config['virtual_coils']; 0: off)")


def apply_virtual_coils_flag(config: dict, opts) -> dict:
    if getattr(opts, "virtual_coils", None) is not None:
        config["virtual_coils"] = opts.virtual_coils
    return config
