"""Kaiser-Bessel gridding on the MI355X (csrc/inr_nufft.hip): trajectory.nufft / nufft_adjoint against
their fp64 restatements nufft_numpy / nufft_adjoint_numpy (same taps, same apodisation, numpy.fft).  Criterion, for every
output: |device - restatement| <= nufft_error_bound / nufft_adjoint_error_bound, the worst-case fp32 rounding bounds derived
in DESIGN (J^2 tap terms or M spread terms, 4 roundings per FFT stage, apodisation, scaling) -- not fitted tolerances.  A
wrong tap, wrap, bin or centre is an error of the order of the normalisation itself, 10^4 bounds or more."""
import ctypes

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import trajectory as T
import nufft_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _pairs(z):
    return torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], -1), dtype=np.float32))


def _complex(t):
    return torch.view_as_complex(t.cpu().contiguous()).numpy().astype(np.complex128)


@pytest.fixture(scope="module")
def forward_refs():
    """nufft_numpy of every (shape, count), computed once and left unchanged"""
    ref = {}
    for (C, H, W) in K.SHAPES:
        img = K.images(C, H, W)
        for M in K.COUNTS:
            pos = K.positions(H, W, M, seed=M)
            ref[(C, H, W, M)] = (img, pos, T.nufft_numpy(img, pos), T.nufft_error_bound(img, pos))
    return ref


@pytest.fixture(scope="module")
def adjoint_refs():
    ref = {}
    for (C, H, W) in K.SHAPES:
        for M in K.COUNTS:
            pos = K.positions(H, W, M, seed=M)
            for name, val in K.samples(C, M).items():
                for weighted in (False, True):
                    w = K.weights(M) if weighted else None
                    ref[(C, H, W, name, M, weighted)] = (val, pos, w, T.nufft_adjoint_numpy(val, pos, H, W, w),
                                                         T.nufft_adjoint_error_bound(val, pos, w, H, W))
    return ref


@pytest.mark.parametrize("M", K.COUNTS)
@pytest.mark.parametrize("C,H,W", K.SHAPES)
def test_forward_against_the_restatement(dev, forward_refs, C, H, W, M):
    img, pos, want, bound = forward_refs[(C, H, W, M)]
    d_img = _pairs(img).to(dev)
    out = T.nufft(d_img, pos)
    assert out.shape == (C, M, 2) and out.dtype == torch.float32 and out.is_cuda
    err = np.abs(_complex(out) - want)
    print("forward %dx%dx%d M=%d: max |out - ref| / bound = %.4f" % (C, H, W, M, (err / bound[:, None]).max()))
    assert (err <= bound[:, None]).all()
    # two calls give the same bits (also: a device tensor of positions, a caller's scratch with a guard behind it)
    need = T.nufft_scratch_floats(C, H, W, M)
    scratch = torch.full((need + 64,), float("nan"), device=dev)
    again = T.nufft(d_img, torch.from_numpy(pos).to(dev), scratch=scratch[:need],
                    apod=T.nufft_device_apodisation(H, W, dev))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    assert torch.isnan(scratch[need:]).all()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("M", K.COUNTS)
@pytest.mark.parametrize("name", ["normal", "single"])
@pytest.mark.parametrize("C,H,W", K.SHAPES)
def test_adjoint_against_the_restatement(dev, adjoint_refs, C, H, W, name, M, weighted):
    val, pos, w, want, bound = adjoint_refs[(C, H, W, name, M, weighted)]
    d_val = _pairs(val).to(dev)
    out = T.nufft_adjoint(d_val, pos, (H, W), w)
    assert out.shape == (C, H, W, 2) and out.dtype == torch.float32 and out.is_cuda
    err = np.abs(_complex(out) - want)
    print("adjoint %s %dx%dx%d M=%d %s: max |out - ref| / bound = %.4f"
          % (name, C, H, W, M, "weighted" if weighted else "w null", (err / bound[:, None, None]).max()))
    assert (err <= bound[:, None, None]).all()
    need = T.nufft_scratch_floats(C, H, W, M)
    scratch = torch.full((need + 64,), float("nan"), device=dev)
    again = T.nufft_adjoint(d_val, torch.from_numpy(pos).to(dev), (H, W), None if w is None else torch.from_numpy(w).to(dev),
                            scratch=scratch[:need], bins=T.nufft_device_bins(pos, H, W, dev))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    assert torch.isnan(scratch[need:]).all()


@pytest.mark.parametrize("C,H,W,M", [(3, 7, 8, 65), (1, 70, 66, 257)])
def test_all_samples_in_one_cell(dev, C, H, W, M):
    """one bin longer than the 64-sample LDS chunk, every other bin empty"""
    pos = K.one_cell(H, W, M, seed=M)
    bin_start, _ = T.nufft_bins(pos, H, W)
    assert int(np.diff(bin_start).max()) == M and int((np.diff(bin_start) > 0).sum()) == 1
    val, w = K.samples(C, M)["normal"], K.weights(M)
    got = _complex(T.nufft_adjoint(_pairs(val).to(dev), pos, (H, W), w))
    bound = T.nufft_adjoint_error_bound(val, pos, w, H, W)
    err = np.abs(got - T.nufft_adjoint_numpy(val, pos, H, W, w))
    print("one cell %dx%dx%d M=%d: max |out - ref| / bound = %.4f" % (C, H, W, M, (err / bound[:, None, None]).max()))
    assert (err <= bound[:, None, None]).all()
    img = K.images(C, H, W)
    err = np.abs(_complex(T.nufft(_pairs(img).to(dev), pos)) - T.nufft_numpy(img, pos))
    assert (err <= T.nufft_error_bound(img, pos)[:, None]).all()


@pytest.mark.parametrize("C,H,W", K.SHAPES)
def test_integer_positions_are_close_to_the_device_inverse_fft(dev, C, H, W):
    """w null, every integer grid point once: ifft2c up to the approximation error measured on the host (section 4.21:
    2.998e-06 of sum |val| / sqrt(H W), threshold 4 x) plus the rounding bound"""
    from inr_mi355x.evalchain import ifft2c
    k = K.images(C, H, W)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pos = np.stack([yy.ravel(), xx.ravel()], axis=1)
    d_k = _pairs(k).to(dev)
    got = _complex(T.nufft_adjoint(d_k.reshape(C, H * W, 2), pos, (H, W)))
    want = _complex(ifft2c(d_k))
    scale = np.abs(k.astype(np.complex128)).reshape(C, -1).sum(axis=1) / np.sqrt(H * W)
    tol = 4 * 2.998e-06 * scale + T.nufft_adjoint_error_bound(k.reshape(C, -1), pos, None, H, W) \
        + T.adjoint_error_bound(k.reshape(C, -1), None, H, W)  # the last: hipFFT's own error in the comparison
    assert (np.abs(got - want) <= tol[:, None, None]).all()


def test_outputs_are_written_nowhere_else(dev):
    """70 x 66, M = 257: partial tiles on both edges of the grid, a partial last chunk; NaN guards behind grid, out and
    the image stay NaN, and every element in front of them is written"""
    C, H, W, M = 1, 70, 66, 257
    lib, st = L.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos = torch.from_numpy(K.positions(H, W, M, seed=M)).to(dev)
    val, w = _pairs(K.samples(C, M)["normal"]).to(dev), torch.from_numpy(K.weights(M)).to(dev)
    img = _pairs(K.images(C, H, W)).to(dev)
    ay, ax = T.nufft_device_apodisation(H, W, dev)
    bin_start, order = T.nufft_device_bins(pos, H, W, dev)
    scratch = torch.empty(T.nufft_scratch_floats(C, H, W, M), device=dev)
    ng, no, ni = C * 4 * H * W * 2, C * M * 2, C * H * W * 2
    grid = torch.full((ng + 256,), float("nan"), device=dev)
    L.check(lib.inr_nufft_prepare(img.data_ptr(), ay.data_ptr(), ax.data_ptr(), C, H, W, grid.data_ptr(), st))
    assert torch.isfinite(grid[:ng]).all() and torch.isnan(grid[ng:]).all()
    assert int((grid[:ng] != 0).sum()) == ni  # the image, centred; zero around it
    out = torch.full((no + 256,), float("nan"), device=dev)
    L.check(lib.inr_nufft_interp(grid.data_ptr(), pos.data_ptr(), C, H, W, M, out.data_ptr(), scratch.data_ptr(),
                                 scratch.numel(), st))
    assert torch.isfinite(out[:no]).all() and torch.isnan(out[no:]).all()
    grid.fill_(float("nan"))
    L.check(lib.inr_nufft_spread(val.data_ptr(), pos.data_ptr(), w.data_ptr(), bin_start.data_ptr(), order.data_ptr(), C,
                                 H, W, M, grid.data_ptr(), scratch.data_ptr(), scratch.numel(), st))
    assert torch.isfinite(grid[:ng]).all() and torch.isnan(grid[ng:]).all()
    back = torch.full((ni + 256,), float("nan"), device=dev)
    L.check(lib.inr_nufft_finish(grid.data_ptr(), ay.data_ptr(), ax.data_ptr(), C, H, W, back.data_ptr(), st))
    assert torch.isfinite(back[:ni]).all() and torch.isnan(back[ni:]).all()


@pytest.mark.parametrize("C,H,W,M", [(3, 7, 8, 65), (2, 40, 36, 257), (1, 70, 66, 63)])
def test_device_adjointness(dev, C, H, W, M):
    """<y, A x> and <A^H y, x>, inner products in fp64 on the host: each device result is within its own bound of its
    restatement, and the restatements are exact transposes, so the two differ by at most
    ||x||_1 max(adjoint bound) + ||y||_1 max(forward bound)"""
    x, y = K.images(C, H, W), K.samples(C, M)["normal"]
    pos = K.positions(H, W, M, seed=M)
    ax = _complex(T.nufft(_pairs(x).to(dev), pos))
    ahy = _complex(T.nufft_adjoint(_pairs(y).to(dev), pos, (H, W)))
    x64, y64 = x.astype(np.complex128), y.astype(np.complex128)
    lhs, rhs = np.vdot(y64, ax), np.vdot(ahy, x64)
    tol = np.abs(x64).sum() * T.nufft_adjoint_error_bound(y, pos, None, H, W).max() \
        + np.abs(y64).sum() * T.nufft_error_bound(x, pos).max()
    print("%dx%dx%d M=%d: |<y, A x> - <A^H y, x>| / tolerance = %.4f" % (C, H, W, M, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol


def test_invalid_arguments_are_refused_before_any_launch(dev):
    C, H, W, M = 2, 7, 8, 65
    lib, st = L.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos = torch.from_numpy(K.positions(H, W, M, seed=M)).to(dev)
    val, w = _pairs(K.samples(C, M)["normal"]).to(dev), torch.from_numpy(K.weights(M)).to(dev)
    ay, ax = T.nufft_device_apodisation(H, W, dev)
    bin_start, order = T.nufft_device_bins(pos, H, W, dev)
    need = T.nufft_scratch_floats(C, H, W, M)
    assert need == 14 * 128
    scratch = torch.full((need + 4,), float("nan"), device=dev)
    grid = torch.full((C * 4 * H * W * 2 + 4,), float("nan"), device=dev)
    img = torch.full((C * H * W * 2 + 4,), float("nan"), device=dev)
    out = torch.full((C * M * 2 + 4,), float("nan"), device=dev)
    p = lambda t, off=0: t.data_ptr() + off  # noqa: E731
    n = ctypes.c_int64(0)

    def refused(rc):
        assert rc == -1  # INR_ERR_INVALID

    for bad in ((0, H, W, M), (33, H, W, M), (C, 2, W, M), (C, H, 2, M), (C, 1 << 16, 1 << 15, M), (C, H, W, 0),
                (C, H, W, 1 << 31)):
        refused(lib.inr_nufft_scratch(*bad, ctypes.byref(n)))
    refused(lib.inr_nufft_scratch(C, H, W, M, None))

    def prepare(i=p(img), y=p(ay), x=p(ax), c=C, h=H, w_=W, g=p(grid)):
        return lib.inr_nufft_prepare(i, y, x, c, h, w_, g, st)

    def finish(g=p(grid), y=p(ay), x=p(ax), c=C, h=H, w_=W, o=p(img)):
        return lib.inr_nufft_finish(g, y, x, c, h, w_, o, st)

    for call in (prepare, finish):
        for kw in (dict(y=None), dict(x=None), dict(c=0), dict(c=33), dict(h=2), dict(w_=2), dict(g=p(grid, 8)),
                   dict(y=p(ay) + 2)):
            refused(call(**kw))
    refused(prepare(i=None)), refused(prepare(g=None)), refused(prepare(i=p(img, 4))), refused(prepare(i=p(grid, 64)))
    refused(finish(g=None)), refused(finish(o=None)), refused(finish(o=p(img, 4))), refused(finish(o=p(grid, 64)))

    def interp(g=p(grid), ps=p(pos), c=C, h=H, w_=W, m=M, o=p(out), s=p(scratch), sf=need):
        return lib.inr_nufft_interp(g, ps, c, h, w_, m, o, s, sf, st)

    for kw in (dict(g=None), dict(ps=None), dict(o=None), dict(s=None), dict(c=0), dict(h=2), dict(m=0), dict(o=p(out, 4)),
               dict(ps=p(pos, 4)), dict(g=p(grid, 8)), dict(s=p(scratch, 8)), dict(sf=need - 1), dict(o=p(grid, 64)),
               dict(o=p(pos)), dict(s=p(grid)), dict(s=p(out)), dict(s=p(pos))):
        refused(interp(**kw))

    def spread(v=p(val), ps=p(pos), w_=p(w), b=p(bin_start), o=p(order), c=C, h=H, wd=W, m=M, g=p(grid), s=p(scratch),
               sf=need):
        return lib.inr_nufft_spread(v, ps, w_, b, o, c, h, wd, m, g, s, sf, st)

    for kw in (dict(v=None), dict(ps=None), dict(b=None), dict(o=None), dict(g=None), dict(s=None), dict(c=33), dict(wd=2),
               dict(m=0), dict(v=p(val, 4)), dict(w_=p(w) + 2), dict(b=p(bin_start) + 2), dict(g=p(grid, 8)),
               dict(s=p(scratch, 4)), dict(sf=need - 1), dict(g=p(val)), dict(g=p(pos)), dict(s=p(val)), dict(s=p(order)),
               dict(s=p(grid))):
        refused(spread(**kw))
    torch.cuda.synchronize()
    # nothing ran: every buffer is as it was
    for t in (scratch, grid, img, out):
        assert torch.isnan(t).all()
    assert spread(w_=None) == 0 and interp(g=p(grid)) == 0  # the good calls go through (w null included)
    torch.cuda.synchronize()


def test_host_visible_bins_are_checked(dev):
    """bin_start in pinned host memory: one that does not start at 0, is not monotone or does not end at M is refused
    before any launch; the right one is read by the kernel from where it is and gives the bits of the device copy"""
    C, H, W, M = 1, 70, 66, 257
    lib, st = L.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos_np = K.positions(H, W, M, seed=M)
    pos, val = torch.from_numpy(pos_np).to(dev), _pairs(K.samples(C, M)["normal"]).to(dev)
    bin_start, order = T.nufft_bins(pos_np, H, W)
    d_order = torch.from_numpy(order).to(dev)
    scratch = torch.empty(T.nufft_scratch_floats(C, H, W, M), device=dev)
    grid = torch.full((C * 4 * H * W * 2,), float("nan"), device=dev)

    def spread(b):
        return lib.inr_nufft_spread(val.data_ptr(), pos.data_ptr(), None, b.data_ptr(), d_order.data_ptr(), C, H, W, M,
                                    grid.data_ptr(), scratch.data_ptr(), scratch.numel(), st)

    full = int(np.flatnonzero(np.diff(bin_start) > 0)[0])  # a bin that holds samples
    for index, value in ((0, 1), (full + 1, int(bin_start[full]) - 1), (len(bin_start) - 1, M - 1)):
        pinned = torch.from_numpy(bin_start.copy()).pin_memory()
        pinned[index] = value
        assert spread(pinned) == -1
    torch.cuda.synchronize()
    assert torch.isnan(grid).all()
    pinned = torch.from_numpy(bin_start.copy()).pin_memory()
    assert spread(pinned) == 0
    torch.cuda.synchronize()
    from_host = grid.clone()
    assert spread(torch.from_numpy(bin_start).to(dev)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(grid).all() and torch.equal(from_host.view(torch.int32), grid.view(torch.int32))
