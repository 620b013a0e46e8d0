"""Kaiser-Bessel gridding on the host (inr_mi355x/trajectory.py; no GPU): the fp64 restatements
nufft_numpy / nufft_adjoint_numpy against the exact operators, their transposition, the apodisation's closed form, the cell
list of the spread kernel, the baseline under operator="gridding", and the switch.

The approximation error of sigma = 2, J = 6 cannot be derived here; it was measured against the exact fp64 operators on the
cases below, normalised by sum |I| / sqrt(H W) (forward) and sum |w val| / sqrt(H W) (adjoint):
    forward 4.184e-06, adjoint 2.998e-06 (Beatty's analysis predicts the order of 1e-5)
and the thresholds are 4 x these (the error depends on the fractional offsets, and the cases sample few of them)."""
import argparse
import math
import os
import re

import numpy as np
import pytest

from inr_mi355x import _lib as L
from inr_mi355x import trajectory as T
from inr_mi355x.synthetic import make_kspace
import nufft_cases as K

FORWARD_MEASURED, ADJOINT_MEASURED = 4.184e-06, 2.998e-06
# |f_gridding - f_exact| / f_exact of the objective after iterations 1..8 of the baseline case below, as measured
CG_MEASURED = [3.039e-06, 8.599e-07, 3.380e-06, 1.067e-06, 1.882e-06, 1.310e-06, 4.069e-06, 1.318e-05]

TRAJECTORIES = {"spokes-13-20": lambda H, W: T.spokes(H, W, 13, 20), "random": lambda H, W: K.positions(H, W, 257, seed=257)}


@pytest.mark.parametrize("traj", sorted(TRAJECTORIES))
@pytest.mark.parametrize("C,H,W", K.HOST_SHAPES)
def test_approximation_error_against_the_exact_operators(C, H, W, traj):
    pos = TRAJECTORIES[traj](H, W)
    M = pos.shape[0]
    img = K.images(C, H, W).astype(np.complex128)
    err = np.abs(T.nufft_numpy(img, pos) - T.nudft_numpy(img, pos)).max(axis=1)
    ratio_f = (err / (np.abs(img).reshape(C, -1).sum(axis=1) / math.sqrt(H * W))).max()
    val = K.samples(C, M)["normal"].astype(np.complex128)
    ratio_a = 0.0
    for w in (None, K.weights(M).astype(np.float64)):
        err = np.abs(T.nufft_adjoint_numpy(val, pos, H, W, w) - T.nudft_adjoint_numpy(val, pos, H, W, w)).reshape(C, -1).max(axis=1)
        scale = (np.abs(val) * (1.0 if w is None else w[None, :])).sum(axis=1) / math.sqrt(H * W)
        ratio_a = max(ratio_a, (err / scale).max())
    print("%dx%dx%d %s: forward %.3e, adjoint %.3e" % (C, H, W, traj, ratio_f, ratio_a))
    assert ratio_f <= 4 * FORWARD_MEASURED and ratio_a <= 4 * ADJOINT_MEASURED
    assert 4 * FORWARD_MEASURED < 1e-3 and 4 * ADJOINT_MEASURED < 1e-3


@pytest.mark.parametrize("C,H,W", K.HOST_SHAPES)
def test_restatements_are_exact_transposes(C, H, W):
    pos = K.positions(H, W, 65, seed=65)
    x = K.images(C, H, W).astype(np.complex128)
    y = K.samples(C, 65)["normal"].astype(np.complex128)
    ax, ahy = T.nufft_numpy(x, pos), T.nufft_adjoint_numpy(y, pos, H, W)
    lhs, rhs = np.vdot(y, ax), np.vdot(ahy, x)
    tol = 1e-12 * (np.linalg.norm(x) * np.linalg.norm(ahy) + np.linalg.norm(y) * np.linalg.norm(ax))
    assert abs(lhs - rhs) <= tol
    # with weights: A^H W y
    w = K.weights(65).astype(np.float64)
    assert abs(np.vdot(w[None, :] * y, ax) - np.vdot(T.nufft_adjoint_numpy(y, pos, H, W, w), x)) <= 4 * tol


def test_integer_positions_approximate_the_inverse_fft():
    C, H, W = 2, 7, 8
    k = K.images(C, H, W).astype(np.complex128)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pos = np.stack([yy.ravel(), xx.ravel()], axis=1)
    got = T.nufft_adjoint_numpy(k.reshape(C, -1), pos, H, W)
    want = T._fftc_numpy(k, True)
    scale = np.abs(k).reshape(C, -1).sum(axis=1) / math.sqrt(H * W)
    assert (np.abs(got - want).reshape(C, -1).max(axis=1) <= 4 * ADJOINT_MEASURED * scale).all()


@pytest.mark.parametrize("n", [3, 5, 6, 40])
def test_apodisation_closed_form_against_quadrature(n):
    """a(nu) = integral of kb(t) cos(2 pi nu t) over |t| <= 3 by Simpson's rule on 2^16 intervals (kb is smooth inside and
    its end value 1 / I0(beta) = 9e-6 is part of the integrand: error far below 1e-9); the fp32 storage rounds by 2^-24"""
    t = np.linspace(-T.NUFFT_TAPS / 2, T.NUFFT_TAPS / 2, (1 << 16) + 1)
    kb = T.nufft_kernel(t)
    simpson = np.ones_like(t)
    simpson[1:-1:2], simpson[2:-1:2] = 4.0, 2.0
    simpson *= (t[1] - t[0]) / 3.0
    a = T.nufft_apodisation(n)
    assert a.dtype == np.float32 and a.shape == (n,)
    for y in range(n):
        nu = (y - n // 2) / (2.0 * n)
        want = float((simpson * kb * np.cos(2.0 * np.pi * nu * t)).sum())
        assert abs(float(a[y]) - want) <= (2.0 ** -24 + 1e-9) * want
    assert T.nufft_kernel(np.array([3.0001, -3.0001, 0.0])).tolist() == [0.0, 0.0, 1.0]
    assert abs(T.NUFFT_BETA - 13.8551) < 1e-4


def test_taps():
    """j0 = ceil(g - 3); six weights kb(g - j) in fp32; an integer g has its peak on the fourth tap"""
    j0, w = T.nufft_taps(np.array([0.0, 2.0, 2.25, 4.0, -1.0, 5.0 + 0.5]), 5)  # c = 2, G = 10: g = 1, 5, 5.5, 9, 9, 2
    assert j0.tolist() == [-2, 2, 3, 6, 6, -1] and w.dtype == np.float32 and w.shape == (6, 6)
    assert w[1].argmax() == 3 and w[1, 3] == 1.0 and np.array_equal(w[3], w[4])
    assert np.allclose(w[2], w[2][::-1])  # g = 5.5: symmetric taps


@pytest.mark.parametrize("H,W", [(6, 5), (7, 8)])
def test_bins_reach_every_tap_by_brute_force(H, W):
    pos = np.concatenate([K.positions(H, W, 257, seed=3), K.one_cell(H, W, 70, seed=4)])
    M = pos.shape[0]
    bin_start, order = T.nufft_bins(pos, H, W)
    Gy, Gx = 2 * H, 2 * W
    nby, nbx = -(-Gy // T.NUFFT_TILE), -(-Gx // T.NUFFT_TILE)
    assert bin_start.dtype == np.int32 and order.dtype == np.int32 and bin_start.shape == (nby * nbx + 1,)
    assert sorted(order.tolist()) == list(range(M))  # a permutation
    assert bin_start[0] == 0 and bin_start[-1] == M and (np.diff(bin_start) >= 0).all()
    bin_of = np.empty(M, dtype=np.int64)
    for b in range(nby * nbx):
        members = order[bin_start[b]:bin_start[b + 1]]
        assert (np.diff(members) > 0).all()  # stable: ascending sample index inside a bin
        bin_of[members] = b
    jy, _ = T.nufft_taps(pos[:, 0], H)
    jx, _ = T.nufft_taps(pos[:, 1], W)
    for m in range(M):
        for ky in range(T.NUFFT_TAPS):
            for kx in range(T.NUFFT_TAPS):
                cy, cx = (jy[m] + ky) % Gy, (jx[m] + kx) % Gx
                reach_y = T.nufft_tile_bins(cy // T.NUFFT_TILE, Gy)
                reach_x = T.nufft_tile_bins(cx // T.NUFFT_TILE, Gx)
                assert bin_of[m] // nbx in reach_y and bin_of[m] % nbx in reach_x


@pytest.mark.parametrize("G", [6, 10, 16, 18, 34, 50, 132, 140])
def test_tile_bins_are_few_ascending_and_complete(G):
    nb = -(-G // T.NUFFT_TILE)
    for tile in range(nb):
        bins = T.nufft_tile_bins(tile, G)
        assert bins == sorted(set(bins)) and len(bins) <= 4 and tile in bins
        lo, hi = tile * T.NUFFT_TILE, min(tile * T.NUFFT_TILE + 15, G - 1)
        for f in range(G):  # a sample with floor(g) = f touches cells f - 3 .. f + 3
            if any(lo <= (f + d) % G <= hi for d in range(-3, 4)):
                assert f // T.NUFFT_TILE in bins


def test_cg_baseline_numpy_under_gridding():
    import torch
    from inr_mi355x.evalchain import ifft2c
    image, _, shape = make_kspace(2, 32, 32)
    C, H, W = shape
    pos, w = T.spokes(H, W, 12), T.density_ramp(12, 32, H, W)
    img = torch.view_as_complex(ifft2c(image.reshape(C, H, W, 2)).contiguous()).numpy().astype(np.complex128)
    y = T.nudft_numpy(img, pos)
    it_e, f_e = T.cg_baseline_numpy(y, pos, shape, w, 8)
    it_g, f_g = T.cg_baseline_numpy(y, pos, shape, w, 8, operator="gridding")
    assert len(it_g) == 8 and len(f_g) == 9 and f_g[0] == f_e[0]
    rel = [abs(a - b) / a for a, b in zip(f_e[1:], f_g[1:])]
    print("relative difference of the objective per iterate:", ", ".join("%.3e" % r for r in rel))
    assert all(r <= 4 * m for r, m in zip(rel, CG_MEASURED))
    same = T.cg_baseline_numpy(y, pos, shape, w, 2, operator="exact")
    assert same[1] == f_e[:3]
    with pytest.raises(ValueError):
        T.cg_baseline_numpy(y, pos, shape, w, 2, operator="kb")


def test_error_bounds_have_the_stated_form():
    C, H, W, M = 2, 40, 36, 65
    pos = K.positions(H, W, M, seed=M)
    img, val, w = K.images(C, H, W), K.samples(C, M)["normal"], K.weights(M)
    u, stages = 2.0 ** -24, 4 * (math.ceil(math.log2(80)) + math.ceil(math.log2(72)))
    S = T._nufft_tap_sum(pos, H, W)
    D = 2.0 / (T.nufft_apodisation(H).astype(np.float64)[:, None] * T.nufft_apodisation(W).astype(np.float64)[None, :])
    n = 36 + 9 + stages
    want = n * u / (1 - n * u) * S * (np.abs(img.astype(np.complex128)) * D[None]).reshape(C, -1).sum(axis=1) / math.sqrt(80 * 72)
    assert np.allclose(T.nufft_error_bound(img, pos), want, rtol=1e-12)
    n = M + 9 + stages
    total = (np.abs(val.astype(np.complex128)) * w.astype(np.float64)[None, :]).sum(axis=1)
    want = n * u / (1 - n * u) * D.max() * S * total / math.sqrt(80 * 72)
    assert np.allclose(T.nufft_adjoint_error_bound(val, pos, w, H, W), want, rtol=1e-12)
    assert 3.5 < S < 4.5  # (sum of six taps)^2 is about a(0)^2 = 4.08


def test_shapes_below_three_points_are_refused():
    pos = np.array([[0.0, 0.0]])
    with pytest.raises(ValueError):
        T.nufft_numpy(np.zeros((1, 2, 5), dtype=np.complex128), pos)
    with pytest.raises(ValueError):
        T.nufft_bins(pos, 5, 2)


# ---- the switch ------------------------------------------------------------------------------------------------------
def test_parse_operator():
    assert T.parse_operator(None) is None
    assert T.parse_operator("exact") == "exact" and T.parse_operator("gridding") == "gridding"
    for bad in ("none", "Gridding", "kb", "", 1, True):
        with pytest.raises(ValueError):
            T.parse_operator(bad)


def test_cli_flag():
    ap = argparse.ArgumentParser()
    T.add_baseline_flags(ap)
    opts = ap.parse_args(["--trajectory-baseline", "cg-3", "--trajectory-operator", "gridding"])
    cfg = T.apply_baseline_flags({}, opts)
    assert cfg == {"trajectory_baseline": "cg-3", "trajectory_operator": "gridding"}
    assert "trajectory_operator" not in T.apply_baseline_flags({}, ap.parse_args([]))


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=500, max_epoch=1, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("extra", [dict(trajectory_operator="kb", trajectory_baseline="cg-2"),
                                   dict(trajectory_operator="gridding"),
                                   dict(trajectory_operator="gridding", trajectory_baseline="none"),
                                   dict(trajectory_operator="exact")])
def test_trainer_refuses_before_anything_is_allocated(extra):
    """a wrong word, or the key without a baseline: ValueError out of _init_fit, on a host that has no device at all"""
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 32, 32)
    with pytest.raises(ValueError, match="trajectory_operator"):
        INRTrainer(_cfg(trajectory="spokes-12", **extra), image, coords, shape, "cuda:0", seed=3)


def test_abi_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "inr_abi.h")).read()
    for name in ("inr_nufft_scratch", "inr_nufft_prepare", "inr_nufft_interp", "inr_nufft_spread", "inr_nufft_finish"):
        assert re.search(r"^int %s\(" % name, text, re.M) and name in L.SYMBOLS
        assert getattr(L.load(), name) is not None
    assert int(re.search(r"^#define INR_NUFFT_TILE (\d+)", text, re.M).group(1)) == T.NUFFT_TILE
    assert int(re.search(r"^#define INR_NUFFT_TAPS (\d+)", text, re.M).group(1)) == T.NUFFT_TAPS
    makefile = open(os.path.join(root, "mri-implicit-neural-representations_amd", "csrc", "Makefile")).read()
    assert "inr_nufft.hip" in makefile
