"""The coordinate grid's own definition (inr_mi355x/grid.py::grid_rows_numpy) on the host: the axis
formula's properties, the row order, coil subsets, the resolution rule of a rendering and the argument errors of
``python -m inr_mi355x.reconstruct`` -- none of it touches a GPU."""
import numpy as np
import pytest
import torch

from inr_mi355x.grid import GridSpec, axis_values_numpy, grid_rows_numpy, resolve_size
from inr_mi355x.synthetic import create_coords

N_LIST = [1, 2, 3, 7, 8, 15, 16, 17, 368, 640]
WINDOWS = [(-1.0, 1.0), (-0.5, 0.25), (0.1, 0.7)]


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("window", WINDOWS)
def test_axis_endpoints_symmetry_monotone(n, window):
    a, b = window
    v = axis_values_numpy(np.arange(n), a, b, n)
    assert v.dtype == np.float32 and v.shape == (n,)
    assert v[0] == np.float32(a)
    if n > 1:
        assert v[-1] == np.float32(b)
    if a == -b and n > 1:  # (a single point is the window's start by definition, as linspace's: it has no mirror image)
        assert np.array_equal(v, -v[::-1])
    assert np.all(np.diff(v) >= 0)


@pytest.mark.parametrize("n", N_LIST)
def test_axis_close_to_linspace_on_full_window(n):
    """<= 1.2e-7 (one fp32 ulp at 1.0) from what create_coords puts on each axis of the full window."""
    ref = create_coords(n, 1, 1)[:, 0].numpy()  # torch.linspace(-1, 1, n)
    got = axis_values_numpy(np.arange(n), -1.0, 1.0, n)
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))))
    print(f"n = {n}: max |v - linspace| = {err:.3g}")
    assert err <= 1.2e-7


def test_whole_grid_close_to_create_coords():
    C, H, W = 3, 17, 8
    got, dist = grid_rows_numpy(GridSpec(C, H, W), 0, C * H * W)
    ref = create_coords(C, H, W).numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) <= 1.2e-7
    want = np.sqrt((got[:, 1] * got[:, 1]).astype(np.float32) + (got[:, 2] * got[:, 2]).astype(np.float32))
    assert dist.dtype == np.float32 and np.array_equal(dist, want.astype(np.float32))


def test_row_order_and_chunks():
    spec = GridSpec(3, 5, 7, window=(-0.5, 0.25, 0.1, 0.7))
    assert spec.rows == 105 and spec.shape == (3, 5, 7)
    whole, dist = grid_rows_numpy(spec, 0, spec.rows)
    z = axis_values_numpy(np.arange(3), -1, 1, 3)
    y = axis_values_numpy(np.arange(5), -0.5, 0.25, 5)
    x = axis_values_numpy(np.arange(7), 0.1, 0.7, 7)
    grid = whole.reshape(3, 5, 7, 3)
    for k in range(3):
        for j in range(5):
            assert np.array_equal(grid[k, j, :, 0], np.full(7, z[k], dtype=np.float32))
            assert np.array_equal(grid[k, j, :, 1], np.full(7, y[j], dtype=np.float32))
            assert np.array_equal(grid[k, j, :, 2], x)
    cuts = [0, 1, 13, 35, 36, 70, 104, 105]
    parts = [grid_rows_numpy(spec, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), dist)
    c0, d0 = grid_rows_numpy(spec, 40, 40)
    assert c0.shape == (0, 3) and d0.shape == (0,)
    with pytest.raises(ValueError):
        grid_rows_numpy(spec, 0, spec.rows + 1)
    with pytest.raises(ValueError):
        grid_rows_numpy(spec, -1, 3)


def test_coil_subset_picks_the_fits_coil_axis():
    C = 15
    spec = GridSpec(C, 4, 3, coils=[0, 7, 14, 7])
    assert spec.shape == (4, 4, 3) and spec.rows == 48
    coords, _ = grid_rows_numpy(spec, 0, spec.rows)
    z = axis_values_numpy(np.arange(C), -1, 1, C)
    assert np.array_equal(coords.reshape(4, 12, 3)[:, :, 0], np.repeat(z[[0, 7, 14, 7]][:, None], 12, axis=1))
    full, _ = grid_rows_numpy(GridSpec(C, 4, 3), 0, C * 12)
    assert np.array_equal(coords[12:24], full[7 * 12:8 * 12])
    one, _ = grid_rows_numpy(GridSpec(1, 2, 2), 0, 4)
    assert np.all(one[:, 0] == -1.0)  # coils_total = 1: the axis is its first point, as linspace(-1, 1, 1)
    with pytest.raises(ValueError):
        grid_rows_numpy(GridSpec(C, 4, 3, coils=[15]), 0, 1)


def test_single_point_axes():
    coords, dist = grid_rows_numpy(GridSpec(2, 1, 1, window=(0.3, 0.9, -0.2, 0.4)), 0, 2)
    assert np.array_equal(coords[:, 1:], np.array([[0.3, -0.2], [0.3, -0.2]], dtype=np.float32))
    assert np.array_equal(coords[:, 0], np.array([-1.0, 1.0], dtype=np.float32))


def test_resolution_rule():
    assert resolve_size(640, 368) == (640, 368)
    assert resolve_size(640, 368, scale=4) == (2560, 1472)
    assert resolve_size(32, 24, scale=2) == (64, 48)
    assert resolve_size(33, 18, scale=0.5) == (17, 9)  # 16.5 -> 17 (nearest, halves up), 9.0
    assert resolve_size(5, 7, scale=0.01) == (1, 1)  # never below 1
    assert resolve_size(33, 18, scale=1.3) == (43, 23)  # 42.9, 23.4
    assert resolve_size(640, 368, height=31) == (31, 368)
    assert resolve_size(640, 368, height=31, width=45, scale=2) == (31, 45)  # height / width override scale
    assert resolve_size(640, 368, width=45, scale=0.5) == (320, 45)
    for bad in (dict(scale=0), dict(scale=-1), dict(scale=float("nan")), dict(height=0), dict(width=-3)):
        with pytest.raises(ValueError):
            resolve_size(640, 368, **bad)


# ---- the command line's argument errors (argparse exits with status 2 before anything is loaded) ----------------------
BASE = ["--config", "c.yaml", "--checkpoint", "m.pt"]


def _parse(*args):
    from inr_mi355x.reconstruct import parse_args
    return parse_args(BASE + list(args))


def test_cli_parses_lists():
    o = _parse("--shape", "2,32,24", "--window", "-0.5,0.25,0.1,0.7", "--coils", "0,3,5", "--radii", "0,0.4,0.8,1.2,5",
               "--scale", "2", "--chunk", "97")
    assert o.shape == [2, 32, 24] and o.window == [-0.5, 0.25, 0.1, 0.7] and o.coils == [0, 3, 5]
    assert o.radii == [0.0, 0.4, 0.8, 1.2, 5.0] and o.scale == 2.0 and o.chunk == 97 and not o.compare
    o = _parse("--synthetic", "2,32,24", "--compare")
    assert o.synthetic == [2, 32, 24] and o.compare and o.shape is None


@pytest.mark.parametrize("args", [
    ("--synthetic", "2,32,24", "--compare", "--window", "-0.5,0.5,-0.5,0.5"),
    ("--synthetic", "2,32,24", "--compare", "--scale", "2"),
    ("--synthetic", "2,32,24", "--compare", "--height", "31"),
    ("--synthetic", "2,32,24", "--compare", "--width", "45"),
    ("--synthetic", "2,32,24", "--compare", "--coils", "0"),
    ("--shape", "2,32,24", "--compare"),
    ("--shape", "2,32,24", "--synthetic", "2,32,24"),
    ("--shape", "2,32"),
    ("--shape", "2,32,x"),
    ("--shape", "2,0,24"),
    ("--window", "0,1,2"),
    ("--window", "0,1,2,three"),
    ("--coils", "0,,2"),
    ("--coils", "0.5"),
    ("--radii", "a,b"),
    ("--scale", "0"),
    ("--height", "0"),
    ("--chunk", "-5"),
])
def test_cli_argument_errors(args, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*args)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_cli_needs_config_and_checkpoint(capsys):
    from inr_mi355x.reconstruct import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--shape", "2,32,24"])
    assert "--config" in capsys.readouterr().err
