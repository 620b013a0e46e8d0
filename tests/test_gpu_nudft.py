"""inr_nudft on the MI355X (csrc/inr_nudft.hip) against the fp64 definition
trajectory.nudft_numpy.  Criterion, for every output:

    |out - ref| <= (H W + 32) 2^-24 sum |I_c| / sqrt(H W)

the worst-case fp32 bound for H W accumulated terms, each formed with a few roundings after an fp64-reduced phase -- not a
fitted tolerance.  A wrong centre, sign or swapped axis is an error of order sum |I_c| / sqrt(H W) itself."""
import math

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import trajectory as T
from inr_mi355x.evalchain import fft2c

pytestmark = pytest.mark.gpu

SHAPES = [(1, 6, 5), (3, 7, 8), (2, 40, 36)]
COUNTS = [1, 63, 65, 257]  # around the 64-sample tile, and several tiles with a partial last one


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _positions(H, W, M, seed):
    """integers, half-integers, the corners 0 and n - 1, values outside the grid and arbitrary fractions"""
    g = np.random.default_rng(seed)
    fixed = [(0.0, 0.0), (H - 1.0, W - 1.0), (0.0, W - 1.0), (H - 1.0, 0.0), (H // 2, W // 2), (0.5, W - 1.5),
             (H - 0.5, -0.5), (-3.0, W + 2.0), (2.0 * H + 1.25, -1.75 * W), (1.0, 2.0), (H / 2 - 0.5, 0.25)]
    pos = np.empty((M, 2), dtype=np.float64)
    for m in range(M):
        if m < len(fixed) and M > 1:
            pos[m] = fixed[m]
        elif m % 3 == 0:
            pos[m] = (g.integers(0, H), g.integers(0, W))
        elif m % 3 == 1:
            pos[m] = (g.integers(0, 2 * H) / 2.0, g.integers(0, 2 * W) / 2.0)
        else:
            pos[m] = (g.uniform(-H, 2 * H), g.uniform(-W, 2 * W))
    if M == 1:
        pos[0] = (H / 2 - 0.5, 0.25)
    return pos


def _images(C, H, W):
    g = np.random.default_rng(C * 100 + H)
    normal = (g.standard_normal((C, H, W)) + 1j * g.standard_normal((C, H, W))).astype(np.complex64)
    delta = np.zeros((C, H, W), dtype=np.complex64)
    for c in range(C):
        delta[c, (H // 2 + 1 + c) % H, (W // 2 - 2 - c) % W] = 1.0  # off the centre, another pixel per coil
    return {"normal": normal, "delta": delta}


def _pairs(z):
    return torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], -1), dtype=np.float32))


def _complex(t):
    return torch.view_as_complex(t.cpu().contiguous()).numpy().astype(np.complex128)


@pytest.fixture(scope="module")
def references():
    """nudft_numpy of every (shape, image, count), computed once and left unchanged"""
    ref = {}
    for (C, H, W) in SHAPES:
        for name, img in _images(C, H, W).items():
            for M in COUNTS:
                pos = _positions(H, W, M, seed=M)
                ref[(C, H, W, name, M)] = (img, pos, T.nudft_numpy(img, pos), T.error_bound(img, H, W))
    return ref


@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("name", ["normal", "delta"])
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_against_the_fp64_definition(dev, references, C, H, W, name, M):
    img, pos, want, bound = references[(C, H, W, name, M)]
    assert np.allclose(bound, (H * W + 32) * 2.0 ** -24 * np.abs(img.astype(np.complex128)).sum(axis=(1, 2)) / math.sqrt(H * W),
                       rtol=1e-15)
    out = T.nudft(_pairs(img).to(dev), pos)
    assert out.shape == (C, M, 2) and out.dtype == torch.float32 and out.is_cuda
    got = _complex(out)
    err = np.abs(got - want)
    print("%s %dx%dx%d M=%d: max |out - ref| / bound = %.4f" % (name, C, H, W, M, (err / bound[:, None]).max()))
    assert (err <= bound[:, None]).all()
    if name == "delta":  # the exact answer is a phasor of modulus 1 / sqrt(H W)
        assert np.abs(np.abs(want) - 1.0 / math.sqrt(H * W)).max() <= 1e-14
    # two calls give the same bits (also: a device tensor of positions, a caller's scratch with a guard behind it)
    need = T.scratch_floats(C, H, W, M)
    scratch = torch.full((need + 64,), float("nan"), device=dev)
    again = T.nudft(_pairs(img).to(dev), torch.from_numpy(pos).to(dev), scratch=scratch[:need])
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    assert torch.isnan(scratch[need:]).all()


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_integer_positions_are_the_device_fft(dev, C, H, W):
    img = _images(C, H, W)["normal"]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pos = np.stack([yy.ravel(), xx.ravel()], axis=1)
    d_img = _pairs(img).to(dev)
    got = _complex(T.nudft(d_img, pos)).reshape(C, H, W)
    want = _complex(fft2c(d_img))
    # hipFFT's own fp32 error is well inside the same bound (O(log(H W)) roundings per output)
    assert (np.abs(got - want) <= T.error_bound(img, H, W)[:, None, None]).all()


def test_output_is_written_nowhere_else(dev):
    """M = 257 on 40 x 36: partial tiles in every blocked dimension (64 samples, 64 rows, 16 columns); the rows behind
    the output stay untouched"""
    C, H, W, M = 2, 40, 36, 257
    img = _images(C, H, W)["normal"]
    pos = torch.from_numpy(_positions(H, W, M, seed=M)).to(dev)
    d_img = _pairs(img).to(dev)
    import ctypes
    buf = torch.full((C * M * 2 + 128,), float("nan"), device=dev)
    scratch = torch.empty(T.scratch_floats(C, H, W, M), device=dev)
    L.check(L.load().inr_nudft(d_img.data_ptr(), C, H, W, pos.data_ptr(), M, buf.data_ptr(), scratch.data_ptr(),
                               scratch.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:C * M * 2]).all() and torch.isnan(buf[C * M * 2:]).all()
    assert torch.equal(buf[:C * M * 2].reshape(C, M, 2), T.nudft(d_img, pos))
