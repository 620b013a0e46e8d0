"""Weighted epochs on the host (no GPU, no library): the numpy restatement of DESIGN.md section 4.23 -- tick rules, the
stratified draw and what follows from its definition -- and the config key with the weights it names."""
import numpy as np
import pytest

from inr_mi355x import sampling as S
from inr_mi355x.shuffle import epoch_order

MAX = 2 ** 32 - 1


def _counts(order, n):
    return np.bincount(order, minlength=n)


def _assert_count_bounds(cdf, order, m):
    """row i is drawn between max(0, q_i // stride - 1) and q_i // stride + 2 times (needs T mod m < stride)"""
    q = np.diff(np.concatenate(([0], cdf.astype(object))))
    total = int(cdf[-1])
    stride = total // m
    assert stride > 0 and total % m < stride
    got = _counts(order, cdf.size)
    for i, c in enumerate(got):
        k = int(q[i]) // stride
        assert max(0, k - 1) <= c <= k + 2, (i, int(c), k)
    assert np.all(got[np.array([int(v) == 0 for v in q])] == 0)


# ---- ticks -------------------------------------------------------------------------------------------------------------
def test_tick_rules():
    w = np.array([np.nan, -1.0, -0.0, 0.0, np.inf, 1.0, 0.5, 3.0, 2.0], dtype=np.float32)
    q = S.row_ticks_numpy(w, 10.0)
    assert q.dtype == np.uint64
    assert q.tolist() == [0, 0, 0, 0, MAX, 10, 5, 30, 20]
    mask = np.array([1, 1, 1, 1, 0, 1, 0, 7, 1], dtype=np.uint8)
    assert S.row_ticks_numpy(w, 10.0, mask).tolist() == [0, 0, 0, 0, 0, 10, 0, 30, 20]
    cdf = S.row_cdf_numpy(w, 10.0, mask)
    assert cdf.dtype == np.uint64 and cdf.tolist() == [0, 0, 0, 0, 0, 10, 10, 40, 60]


def test_ticks_floor_and_clip():
    w = np.array([0.3, 1.0, 2.0, 1e30], dtype=np.float32)
    # fp64(fp32(0.3)) * 10 = 3.0000001192...: floor 3; the product is formed in fp64, not fp32
    assert S.row_ticks_numpy(w, 10.0).tolist() == [3, 10, 20, MAX]
    assert S.row_ticks_numpy(w[:3], S.default_scale(2.0)).tolist() == [int(np.floor(np.float64(np.float32(0.3)) * (MAX / 2.0))),
                                                                       int(np.floor(MAX / 2.0)), MAX]
    assert S.row_ticks_numpy(np.array([1.0], np.float32), float(MAX) + 5.0).tolist() == [MAX]  # clipped, not wrapped
    assert S.default_scale(4.0) == MAX / 4.0


@pytest.mark.parametrize("scale", [0.0, -1.0, np.inf, np.nan])
def test_bad_scale(scale):
    with pytest.raises(ValueError, match="scale"):
        S.row_cdf_numpy(np.ones(3, np.float32), scale)


def test_mask_shape_is_checked():
    with pytest.raises(ValueError, match="mask"):
        S.row_ticks_numpy(np.ones(3, np.float32), 1.0, np.ones(2, np.uint8))


# ---- the draw ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 257, 5000])
def test_equal_weights_full_draw_is_the_shuffle_order(n):
    for scale in (1.0, 1000.0, S.default_scale(1.0)):
        cdf = S.row_cdf_numpy(np.ones(n, np.float32), scale)
        for seed, epoch in ((0, 0), (9, 3), (2 ** 40 + 3, 12)):
            got = S.epoch_draw_numpy(cdf, n, seed, epoch)
            assert got.dtype == np.int64
            assert np.array_equal(got, epoch_order(n, seed, epoch)), (n, scale, seed, epoch)


def test_zero_tick_rows_are_never_drawn():
    rng = np.random.default_rng(1)
    w = rng.random(3000).astype(np.float32)
    w[:100] = 0.0
    w[1000:1500] = -1.0
    w[-50:] = np.nan
    mask = (rng.random(3000) < 0.6).astype(np.uint8)
    cdf = S.row_cdf_numpy(w, S.default_scale(1.0), mask)
    dead = ~((w > 0) & (mask != 0))
    for m in (3000, 1000, 6005, 1):
        order = S.epoch_draw_numpy(cdf, m, 4, 2)
        assert order.shape == (m,) and order.min() >= 0 and order.max() < 3000
        assert not dead[order].any()


@pytest.mark.parametrize("m", [4000, 1333, 8005])
def test_count_bounds_random_weights(m):
    rng = np.random.default_rng(7)
    w = (rng.random(4000) ** 4).astype(np.float32)  # a long tail of light rows
    w[17] = 50.0  # and one dominant row
    cdf = S.row_cdf_numpy(w, S.default_scale(float(w.max())))
    _assert_count_bounds(cdf, S.epoch_draw_numpy(cdf, m, 3, 1), m)


def test_draw_is_a_pure_function_of_seed_and_epoch():
    w = np.random.default_rng(2).random(2000).astype(np.float32)
    cdf = S.row_cdf_numpy(w, S.default_scale(1.0))
    a = S.epoch_draw_numpy(cdf, 2000, 5, 3)
    assert np.array_equal(a, S.epoch_draw_numpy(cdf.copy(), 2000, 5, 3))
    assert not np.array_equal(a, S.epoch_draw_numpy(cdf, 2000, 5, 4))
    assert not np.array_equal(a, S.epoch_draw_numpy(cdf, 2000, 6, 3))
    assert np.array_equal(a, S.epoch_draw_numpy(cdf, 2000, 5 + 2 ** 64, 3 + 2 ** 32))  # seed mod 2^64, epoch mod 2^32


def test_stride_zero_and_empty_total():
    cdf = S.row_cdf_numpy(np.array([0.0, 0.0, 1.0, 0.0, 1.0], np.float32), 1.0)  # T = 2
    assert S.epoch_draw_numpy(cdf, 5, 1, 0).tolist() == [2] * 5  # the row of threshold 0
    assert S.epoch_draw_numpy(np.zeros(4, np.uint64), 3, 1, 0).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        S.epoch_draw_numpy(cdf, 0, 1, 0)
    with pytest.raises(ValueError):
        S.epoch_draw_numpy(cdf, 2 ** 31, 1, 0)


def test_draw_keys_differ_from_the_round_keys():
    from inr_mi355x.shuffle import round_keys
    k = S.draw_keys(3, 4)
    assert len(k) == 2 and all(0 <= v < 2 ** 32 for v in k) and k[0] != k[1]
    assert not set(k) & set(round_keys(3, 4))
    assert k == S.draw_keys(3 + 2 ** 64, 4 + 2 ** 32) and k != S.draw_keys(3, 5) and k != S.draw_keys(4, 4)


# ---- the config key ----------------------------------------------------------------------------------------------------
def test_parse_row_sampling(tmp_path):
    for off in (None, False, "none", "None"):
        assert S.parse_row_sampling(off) is None
    for mode in ("uniform", "density", "ring-inverse"):
        assert S.parse_row_sampling(mode) == mode
    path = str(tmp_path / "w.npy")
    np.save(path, np.ones(4, np.float32))
    assert S.parse_row_sampling(path) == path
    for bad in ("Uniform", "ring_inverse", "weights.npz", "", 3, True, str(tmp_path / "missing.npy")):
        with pytest.raises(ValueError, match="row_sampling"):
            S.parse_row_sampling(bad)


def test_check_row_sampling_refusals():
    base = dict(row_sampling="uniform")
    assert S.check_row_sampling({}, None, True, 4) is None  # key absent: nothing is looked at
    assert S.check_row_sampling(base, None, False, 1) == "uniform"
    with pytest.raises(ValueError, match="graph_steps"):
        S.check_row_sampling(base, None, True, 1)
    with pytest.raises(ValueError, match="per_coil"):
        S.check_row_sampling(dict(base, per_coil=True), None, False, 1)
    with pytest.raises(ValueError, match="use_tv"):
        S.check_row_sampling(dict(base, use_tv=True), None, False, 1)
    with pytest.raises(NotImplementedError, match="LSL"):
        S.check_row_sampling(dict(base, loss="LSL"), None, False, 1)
    with pytest.raises(NotImplementedError, match="rank"):
        S.check_row_sampling(base, None, False, 2)
    with pytest.raises(ValueError, match="trajectory"):
        S.check_row_sampling(dict(row_sampling="density"), None, False, 1)
    assert S.check_row_sampling(dict(row_sampling="density"), ("spokes", 8, 24), False, 1) == "density"


def test_file_weights(tmp_path):
    p = str(tmp_path / "w.npy")
    np.save(p, np.array([0.0, 1.5, 2.0], np.float64))
    w = S.file_weights(p, 3)
    assert w.dtype == np.float32 and w.tolist() == [0.0, 1.5, 2.0]
    np.save(p, np.array([0.0, 1.5, 2.0], np.float32))
    assert S.file_weights(p, 3).tolist() == [0.0, 1.5, 2.0]
    for bad in (np.ones(4, np.float32), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]),
                np.array([1.0, np.inf, 1.0]), np.ones(3, np.int64), np.ones((3, 1), np.float32)):
        np.save(p, bad)
        with pytest.raises(ValueError, match="row_sampling"):
            S.file_weights(p, 3)


def test_density_weights_follow_the_rows_of_trajectory_coords():
    from inr_mi355x.trajectory import density_ramp, parse_trajectory, positions, trajectory_coords
    C, H, W = 3, 24, 20
    traj = parse_trajectory("spokes-8-24")
    w = S.density_weights(traj, C, H, W)
    pos = positions(traj, H, W)
    rows = trajectory_coords(pos, C, H, W).numpy()
    assert w.dtype == np.float32 and w.shape == (rows.shape[0],) == (C * 8 * 24,)
    ramp = density_ramp(8, 24, H, W).astype(np.float32)  # [M], spoke-major
    # row k of coil c is sample k of the trajectory: the same weight in every coil, the ramp along a spoke
    assert np.array_equal(w.reshape(C, 8 * 24), np.broadcast_to(ramp, (C, 8 * 24)))
    per_spoke = w.reshape(C, 8, 24)
    j = np.abs(np.arange(24) - 12).astype(np.float64)
    j[12] = 0.25
    assert np.allclose(per_spoke / per_spoke[0, 0, 0], np.broadcast_to(j / j[0], (C, 8, 24)), rtol=1e-6)
    # ... and the row's own radius orders the weights: the centre sample of every spoke is its lightest row
    centre = trajectory_coords(np.array([[H // 2, W // 2]], np.float64), 1, H, W).numpy()[0]
    radius = np.hypot(rows[:, 1] - centre[1], rows[:, 2] - centre[2]).reshape(C, 8, 24)
    assert np.all(radius.argmin(axis=2) == 12) and np.all(per_spoke.argmin(axis=2) == 12)
    assert S.density_weights(traj, C, H, W, "uniform").std() == 0
    with pytest.raises(ValueError, match="trajectory"):
        S.density_weights(None, C, H, W)


def test_ring_inverse_weights_against_a_hand_table():
    radii = np.array([0.0, 0.25, 0.5, 1.0])
    divisors = np.array([8.0, 2.0, 0.5], np.float32)
    dist = np.array([0.0, 0.1, 0.25, 0.3, 0.5, 0.9, 1.0, 1.4], np.float32)
    w = S.ring_inverse_weights_numpy(dist, radii, divisors)
    # divisor[last] / divisor[r]: lower end included, upper excluded; the outermost ring reaches beyond its radius
    assert w.dtype == np.float32
    assert w.tolist() == [0.0625, 0.0625, 0.25, 0.25, 1.0, 1.0, 1.0, 1.0]
    third = S.ring_inverse_weights_numpy(dist[:2], np.array([0.0, 0.5, 1.0]), np.array([3.0, 1.0], np.float32))
    assert third.tolist() == [float(np.float32(1.0) / np.float32(3.0))] * 2
