"""inr_adjoint_nudft on the MI355X (csrc/inr_nudft_adjoint.hip) against the fp64 definition
trajectory.nudft_adjoint_numpy.  Criterion, for every pixel:

    |out - ref| <= (M + 32) 2^-24 sum_m |w_m val_c[m]| / sqrt(H W)

the worst-case fp32 bound for M accumulated terms, each formed with a few roundings after an fp64-reduced phase -- not a
fitted tolerance.  A wrong centre, sign or swapped axis is an error of order sum |w val| / sqrt(H W) itself."""
import ctypes
import math

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import trajectory as T
from inr_mi355x.evalchain import ifft2c
from test_gpu_nudft import _positions

pytestmark = pytest.mark.gpu

SHAPES = [(1, 6, 5), (3, 7, 8), (2, 40, 36), (1, 70, 66)]  # the last: two tiles in both image dimensions, partial edges
COUNTS = [1, 63, 65, 257]  # around the 16-sample chunk and the 64-sample table padding


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _samples(C, M):
    g = np.random.default_rng(C * 1000 + M)
    normal = (g.standard_normal((C, M)) + 1j * g.standard_normal((C, M))).astype(np.complex64)
    single = np.zeros((C, M), dtype=np.complex64)
    for c in range(C):
        single[c, (M // 2 + c) % M] = 0.75 - 1.25j  # one non-zero sample, another one per coil
    return {"normal": normal, "single": single}


def _weights(M):
    return np.random.default_rng(M).uniform(0.25, 4.0, M).astype(np.float32)


def _pairs(z):
    return torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], -1), dtype=np.float32))


def _complex(t):
    return torch.view_as_complex(t.cpu().contiguous()).numpy().astype(np.complex128)


@pytest.fixture(scope="module")
def references():
    """nudft_adjoint_numpy of every (shape, samples, count, weights), computed once and left unchanged"""
    ref = {}
    for (C, H, W) in SHAPES:
        for M in COUNTS:
            pos = _positions(H, W, M, seed=M)
            for name, val in _samples(C, M).items():
                for weighted in (False, True):
                    w = _weights(M) if weighted else None
                    ref[(C, H, W, name, M, weighted)] = (val, pos, w, T.nudft_adjoint_numpy(val, pos, H, W, w),
                                                         T.adjoint_error_bound(val, w, H, W))
    return ref


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("name", ["normal", "single"])
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_against_the_fp64_definition(dev, references, C, H, W, name, M, weighted):
    val, pos, w, want, bound = references[(C, H, W, name, M, weighted)]
    d_val = _pairs(val).to(dev)
    out = T.nudft_adjoint(d_val, pos, (H, W), w)
    assert out.shape == (C, H, W, 2) and out.dtype == torch.float32 and out.is_cuda
    err = np.abs(_complex(out) - want)
    print("%s %dx%dx%d M=%d %s: max |out - ref| / bound = %.4f"
          % (name, C, H, W, M, "weighted" if weighted else "w null", (err / bound[:, None, None]).max()))
    assert (err <= bound[:, None, None]).all()
    if name == "single":  # the exact answer is a plane wave of modulus |w val| / sqrt(H W)
        for c in range(C):
            m = (M // 2 + c) % M
            mod = abs(complex(val[c, m])) * (float(w[m]) if weighted else 1.0) / math.sqrt(H * W)
            assert np.abs(np.abs(want[c]) - mod).max() <= 1e-14 * max(1.0, mod)
    # two calls give the same bits (also: a device tensor of positions, a caller's scratch with a guard behind it)
    need = T.adjoint_scratch_floats(C, H, W, M)
    scratch = torch.full((need + 64,), float("nan"), device=dev)
    again = T.nudft_adjoint(d_val, torch.from_numpy(pos).to(dev), (H, W), None if w is None else torch.from_numpy(w).to(dev),
                            scratch=scratch[:need])
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    assert torch.isnan(scratch[need:]).all()


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_integer_positions_are_the_device_inverse_fft(dev, C, H, W):
    g = np.random.default_rng(H)
    k = (g.standard_normal((C, H, W)) + 1j * g.standard_normal((C, H, W))).astype(np.complex64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pos = np.stack([yy.ravel(), xx.ravel()], axis=1)
    d_k = _pairs(k).to(dev)
    got = _complex(T.nudft_adjoint(d_k.reshape(C, H * W, 2), pos, (H, W)))
    want = _complex(ifft2c(d_k))
    # hipFFT's own fp32 error is well inside the same bound (O(log(H W)) roundings per output)
    bound = T.adjoint_error_bound(k.reshape(C, -1), None, H, W)
    print("%dx%dx%d: max |adjoint - ifft2c| / bound = %.4f" % (C, H, W, (np.abs(got - want) / bound[:, None, None]).max()))
    assert (np.abs(got - want) <= bound[:, None, None]).all()


def test_output_is_written_nowhere_else(dev):
    """M = 257 on 70 x 66: partial tiles in both image dimensions and a partial last chunk of samples; the floats behind
    the output stay untouched"""
    C, H, W, M = 1, 70, 66, 257
    val = _samples(C, M)["normal"]
    pos = torch.from_numpy(_positions(H, W, M, seed=M)).to(dev)
    w = torch.from_numpy(_weights(M)).to(dev)
    d_val = _pairs(val).to(dev)
    n = C * H * W * 2
    buf = torch.full((n + 256,), float("nan"), device=dev)
    scratch = torch.empty(T.adjoint_scratch_floats(C, H, W, M), device=dev)
    L.check(L.load().inr_adjoint_nudft(d_val.data_ptr(), pos.data_ptr(), w.data_ptr(), C, H, W, M, buf.data_ptr(),
                                       scratch.data_ptr(), scratch.numel(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:n]).all() and torch.isnan(buf[n:]).all()
    assert torch.equal(buf[:n].reshape(C, H, W, 2), T.nudft_adjoint(d_val, pos, (H, W), w))


@pytest.mark.parametrize("C,H,W,M", [(3, 7, 8, 65), (2, 40, 36, 257), (1, 70, 66, 63)])
def test_device_adjointness(dev, C, H, W, M):
    """<y, A x> and <A^H y, x> with A x from T.nudft and A^H y from T.nudft_adjoint, both inner products formed in fp64 on
    the host: each device result is within its own bound of the exact operator's, and the exact operators are adjoint, so
    the two differ by at most ||x||_1 max(adjoint bound) + ||y||_1 max(forward bound)."""
    g = np.random.default_rng(M + H)
    x = (g.standard_normal((C, H, W)) + 1j * g.standard_normal((C, H, W))).astype(np.complex64)
    y = (g.standard_normal((C, M)) + 1j * g.standard_normal((C, M))).astype(np.complex64)
    pos = _positions(H, W, M, seed=M)
    ax = _complex(T.nudft(_pairs(x).to(dev), pos))
    ahy = _complex(T.nudft_adjoint(_pairs(y).to(dev), pos, (H, W)))
    x64, y64 = x.astype(np.complex128), y.astype(np.complex128)
    lhs, rhs = np.vdot(y64, ax), np.vdot(ahy, x64)
    tol = np.abs(x64).sum() * T.adjoint_error_bound(y, None, H, W).max() + np.abs(y64).sum() * T.error_bound(x, H, W).max()
    print("%dx%dx%d M=%d: |<y, A x> - <A^H y, x>| / tolerance = %.4f" % (C, H, W, M, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol
