"""inr_grid_rows on the MI355X (``-m gpu``): bit-equal to the numpy restatement of DESIGN.md section 4.16
(inr_mi355x/grid.py::grid_rows_numpy) -- coordinates and dist, whole grids and chunks, 16-byte aligned and unaligned
buffers -- writes nothing behind its rows, is reproducible, capturable, and refuses bad descriptions before any launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
PAD = 64  # sentinel floats behind each output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _run(spec, lo, hi, dev, with_dist=True, offset=0):
    """grid_rows into views of sentinel-filled buffers (``offset`` floats in front: 0 = 16-byte aligned); checks the
    sentinels in front of and behind the rows, returns (coords, dist) as numpy."""
    from inr_mi355x.grid import grid_rows
    n = hi - lo
    cbuf = torch.full((offset + 3 * n + PAD,), SENTINEL, device=dev)
    dbuf = torch.full((offset + n + PAD,), SENTINEL, device=dev)
    cview = cbuf[offset:offset + 3 * n].view(n, 3)
    dview = dbuf[offset:offset + n]
    c, d = grid_rows(spec, lo, hi, coords_out=cview, dist_out=dview if with_dist else None, with_dist=with_dist)
    assert c.data_ptr() == cview.data_ptr() and (d is None or d.data_ptr() == dview.data_ptr())
    torch.cuda.synchronize()
    assert bool((cbuf[:offset] == SENTINEL).all()) and bool((cbuf[offset + 3 * n:] == SENTINEL).all())
    assert bool((dbuf[:offset] == SENTINEL).all()) and bool((dbuf[offset + n:] == SENTINEL).all())
    if not with_dist:
        assert d is None and bool((dbuf == SENTINEL).all())
    return cview.cpu().numpy(), (dview.cpu().numpy() if with_dist else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(spec, lo, hi, dev, want=None, **kw):
    from inr_mi355x.grid import grid_rows_numpy
    wc, wd = grid_rows_numpy(spec, lo, hi) if want is None else (want[0][lo:hi], want[1][lo:hi])
    gc, gd = _run(spec, lo, hi, dev, **kw)
    assert gc.dtype == np.float32 and np.array_equal(_bits(gc), _bits(wc)), (spec, lo, hi)
    if gd is not None:
        assert np.array_equal(_bits(gd), _bits(wd)), (spec, lo, hi)


def _specs():
    from inr_mi355x.grid import GridSpec
    return {
        "3x5x7": GridSpec(3, 5, 7),
        "subset_window": GridSpec(15, 33, 18, coils=[0, 7, 14], window=(-0.5, 0.25, 0.1, 0.7)),
        "H1": GridSpec(4, 1, 37),
        "W1": GridSpec(4, 37, 1, window=(-1.0, 1.0, 0.3, 0.9)),
        "HW1": GridSpec(3, 1, 1),
        "C1": GridSpec(1, 9, 11),
        "2x640x368": GridSpec(2, 640, 368),
    }


@pytest.mark.parametrize("name", ["3x5x7", "subset_window", "H1", "W1", "HW1", "C1", "2x640x368"])
@pytest.mark.parametrize("offset", [0, 1])
def test_whole_grid_bit_equal(dev, name, offset):
    """offset 1: buffers that are only 4-byte aligned take the kernel's narrow stores"""
    spec = _specs()[name]
    _check(spec, 0, spec.rows, dev, offset=offset)


@pytest.mark.parametrize("name", ["subset_window", "2x640x368"])
def test_chunks_bit_equal(dev, name):
    from inr_mi355x.grid import grid_rows_numpy
    spec = _specs()[name]
    n, plane = spec.rows, spec.H * spec.W
    want = grid_rows_numpy(spec, 0, n)
    chunks = [(13, 1001), (0, 1), (n - 1, 1), (n - 1001, 1001),  # ... ending on the grid's last row
              (plane - 5, 1001),  # spanning a coil boundary
              (plane - 1, 2), (plane, 3), (7, 1024), (7, 1025), (1, 4), (2, 3)]
    for lo, cnt in chunks:
        for offset in (0, 2):
            _check(spec, lo, lo + cnt, dev, want=want, offset=offset)


def test_dist_null(dev):
    for name in ("3x5x7", "subset_window"):
        spec = _specs()[name]
        _check(spec, 0, spec.rows, dev, with_dist=False)
        _check(spec, 13, 13 + 77, dev, with_dist=False, offset=3)


def test_two_calls_identical_bytes_and_allocated_outputs(dev):
    from inr_mi355x.grid import grid_coords, grid_rows, grid_rows_numpy
    spec = _specs()["subset_window"]
    a = grid_rows(spec, 5, 1500, device=dev)
    b = grid_rows(spec, 5, 1500, device=dev)
    assert a[0].shape == (1495, 3) and a[1].shape == (1495,) and a[0].device == dev
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    c, d = grid_rows(spec, 0, spec.rows, with_dist=False, device=dev)
    assert d is None
    # the fit's own grid as one tensor
    full = grid_coords(3, 5, 7, device=dev)
    assert np.array_equal(_bits(full.cpu().numpy()), _bits(grid_rows_numpy(_specs()["3x5x7"], 0, 105)[0]))
    # n_rows == 0 is a successful no-op
    e = grid_rows(spec, 40, 40, device=dev)
    assert e[0].shape == (0, 3) and e[1].shape == (0,)


def test_capturable_one_launch_no_allocation(dev):
    from inr_mi355x.grid import grid_rows, grid_rows_numpy
    spec = _specs()["subset_window"]
    n = spec.rows
    coords = torch.zeros(n, 3, device=dev)
    dist = torch.zeros(n, device=dev)
    grid_rows(spec, 0, n, coords_out=coords, dist_out=dist)  # warm: the code object is loaded outside capture
    torch.cuda.synchronize()
    n_alloc = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    grid_rows(spec, 0, n, coords_out=coords, dist_out=dist)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n_alloc
    coords.zero_()
    dist.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            grid_rows(spec, 0, n, coords_out=coords, dist_out=dist)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert float(coords.abs().sum()) == 0.0  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    wc, wd = grid_rows_numpy(spec, 0, n)
    assert np.array_equal(_bits(coords.cpu().numpy()), _bits(wc)) and np.array_equal(_bits(dist.cpu().numpy()), _bits(wd))


def test_refusals_launch_nothing(dev):
    """Each bad description raises with the library's message; the buffers keep their sentinels."""
    import ctypes as C
    from inr_mi355x import _lib as L
    from inr_mi355x.grid import GridSpec, grid_rows
    coords = torch.full((200, 3), SENTINEL, device=dev)
    dist = torch.full((200,), SENTINEL, device=dev)

    def call(spec, lo, hi):
        n = max(hi - lo, 0)
        return grid_rows(spec, lo, hi, coords_out=coords[:n], dist_out=dist[:n])

    ok = GridSpec(3, 5, 7)
    cases = [
        (GridSpec(3, 0, 7), 0, 1, "must be >= 1"),
        (GridSpec(3, 5, -2), 0, 1, "must be >= 1"),
        (GridSpec(0, 5, 7, coils=[0]), 0, 1, "must be >= 1"),
        (GridSpec(3, 5, 7, coils=[]), 0, 0, "must be >= 1"),
        (GridSpec(70, 1, 1, coils=list(range(65))), 0, 65, "at most 64"),
        (GridSpec(3, 5, 7, coils=[0, 3]), 0, 70, r"coils\[1\] = 3 is outside \[0, 3\)"),
        (GridSpec(3, 5, 7, coils=[-1]), 0, 35, "outside"),
        (GridSpec(3, 5, 7, window=(float("nan"), 1, -1, 1)), 0, 105, "non-finite window"),
        (GridSpec(3, 5, 7, window=(-1, 1, -1, float("inf"))), 0, 105, "non-finite window"),
        (ok, -1, 4, "rows"),
        (ok, 5, 3, "rows"),
        (ok, 100, 106, "rows"),
        (ok, 106, 106, "rows"),
    ]
    for spec, lo, hi, msg in cases:
        with pytest.raises(RuntimeError, match="inr_grid_rows.*" + msg):
            call(spec, lo, hi)
    lib = L.load()
    d = L.GridDesc(coils_total=3, n_coils=1, H=5, W=7, y0=-1, y1=1, x0=-1, x1=1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert lib.inr_grid_rows(None, 0, 1, coords.data_ptr(), None, stream) == -1 and "null" in L.last_error()
    assert lib.inr_grid_rows(C.byref(d), 0, 1, None, dist.data_ptr(), stream) == -1 and "null" in L.last_error()
    assert lib.inr_grid_rows(C.byref(d), 0, 1 << 31, coords.data_ptr(), None, stream) == -1 and "2^31" in L.last_error()
    torch.cuda.synchronize()
    assert bool((coords == SENTINEL).all()) and bool((dist == SENTINEL).all())
    # the wrapper's own refusals
    with pytest.raises(RuntimeError, match="shape"):
        grid_rows(ok, 0, 10, coords_out=coords[:9])
    with pytest.raises(RuntimeError, match="contiguous"):
        grid_rows(ok, 0, 10, coords_out=coords[:10].double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid_rows(ok, 0, 10, coords_out=torch.zeros(10, 3))
