"""The adjoint of the off-grid sampling and the conventional baseline on the host (inr_mi355x/trajectory.py, DESIGN.md
section 4.20): the fp64 definition against nudft_numpy and the centred inverse FFT, the density weights, the switches'
grammar, the library's argument checks on fake pointers, the trainers' refusals and the conjugate-gradient iteration in
fp64.  None of it touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import trajectory as T
from inr_mi355x.evalchain import ifft2c
from inr_mi355x.synthetic import make_kspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_positions(H, W):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([yy.ravel(), xx.ravel()], axis=1)


def _cnormal(g, *shape):
    return g.standard_normal(shape) + 1j * g.standard_normal(shape)


@pytest.mark.parametrize("C,H,W,M", [(1, 6, 5, 7), (3, 7, 8, 65), (2, 40, 36, 257)])
def test_definition_is_the_conjugate_transpose(C, H, W, M):
    g = np.random.default_rng(M)
    pos = np.stack([g.uniform(-H, 2 * H, M), g.uniform(-W, 2 * W, M)], axis=1)  # outside the grid too
    pos[0] = (H - 1.0, 0.0)
    x, y = _cnormal(g, C, H, W), _cnormal(g, C, M)
    lhs, rhs = np.vdot(y, T.nudft_numpy(x, pos)), np.vdot(T.nudft_adjoint_numpy(y, pos, H, W), x)
    print("%dx%dx%d M=%d: |<y, A x> - <A^H y, x>| = %.3g" % (C, H, W, M, abs(lhs - rhs)))
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)
    # weights multiply the samples; pairs are read like complex numbers
    w = g.uniform(0.25, 4.0, M)
    got = T.nudft_adjoint_numpy(np.stack([y.real, y.imag], -1), pos, H, W, w)
    assert got.dtype == np.complex128 and got.shape == (C, H, W)
    assert np.abs(got - T.nudft_adjoint_numpy(y * w[None, :], pos, H, W)).max() <= 1e-13 * np.abs(got).max()
    bound = T.adjoint_error_bound(y, w, H, W)
    assert bound.shape == (C,)
    assert np.allclose(bound, (M + 32) * 2.0 ** -24 * (np.abs(y) * w[None, :]).sum(axis=1) / np.sqrt(H * W), rtol=1e-15)


@pytest.mark.parametrize("H,W", [(6, 5), (7, 8), (5, 7)])
def test_on_the_integer_grid_it_is_the_centred_inverse_fft(H, W):
    g = np.random.default_rng(H * 10 + W)
    k = _cnormal(g, 2, H, W)
    pairs = torch.from_numpy(np.stack([k.real, k.imag], -1))
    want = torch.view_as_complex(ifft2c(pairs)).numpy()
    got = T.nudft_adjoint_numpy(k.reshape(2, -1), _grid_positions(H, W), H, W)
    print("%dx%d: max |adjoint - ifft2c| = %.3g" % (H, W, np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-12


def test_density_ramp():
    w = T.density_ramp(3, 8)
    assert w.dtype == np.float64 and w.shape == (24,)
    assert np.array_equal(w.reshape(3, 8), np.tile([4, 3, 2, 1, 0.25, 1, 2, 3], (3, 1)))
    assert np.array_equal(T.density_ramp(2, 5), np.tile([2, 1, 0.25, 1, 2], 2))  # odd readout: centre at R // 2
    for H, W in ((32, 32), (40, 36)):
        ws = T.density_ramp(13, 20, H, W)
        assert abs(ws.sum() - H * W) <= 1e-9 * H * W
        assert np.allclose(ws / ws[0], T.density_ramp(13, 20) / 10.0, rtol=1e-15)
    assert abs(T.normalise_density(np.array([1.0, 3.0]), 4, 5).sum() - 20.0) <= 1e-12
    for bad in ((0, 8), (3, 1)):
        with pytest.raises(ValueError):
            T.density_ramp(*bad)


def test_parse_density_and_baseline_grammar(tmp_path):
    H, W = 8, 6
    sp = T.parse_trajectory("spokes-3")
    name, w = T.parse_density(None, sp, H, W)
    assert name == "ramp" and np.array_equal(w, T.density_ramp(3, 8, H, W))
    assert T.parse_density("ramp", sp, H, W)[0] == "ramp"
    name, w = T.parse_density("uniform", sp, H, W)
    assert name == "uniform" and np.allclose(w, H * W / 24.0, rtol=1e-15)
    assert T.parse_density("ramp", T.parse_trajectory("spokes-3-10"), H, W)[1].shape == (30,)
    pos_file = tmp_path / "p.npy"
    np.save(pos_file, T.spokes(H, W, 2))
    ft = T.parse_trajectory(str(pos_file))
    assert T.parse_density(None, ft, H, W)[0] == "uniform"
    with pytest.raises(ValueError, match="ramp"):
        T.parse_density("ramp", ft, H, W)
    good = tmp_path / "w.npy"
    np.save(good, np.linspace(1.0, 2.0, 16))
    name, w = T.parse_density(str(good), ft, H, W)
    assert name == str(good) and abs(w.sum() - H * W) <= 1e-9 and np.allclose(w / w[0], np.linspace(1.0, 2.0, 16))
    for fname, arr in (("neg", np.linspace(-1.0, 2.0, 16)), ("zero", np.zeros(16)), ("nan", np.full(16, np.nan)),
                       ("f32", np.ones(16, np.float32)), ("short", np.ones(15)), ("two", np.ones((16, 1)))):
        f = tmp_path / (fname + ".npy")
        np.save(f, arr)
        with pytest.raises(ValueError):
            T.parse_density(str(f), ft, H, W)
    for bad in ("pipe-menon", "voronoi", "", 3, str(tmp_path / "missing.npy")):
        with pytest.raises(ValueError):
            T.parse_density(bad, sp, H, W)
    with pytest.raises(ValueError):
        T.parse_density("uniform", None, H, W)
    assert T.parse_baseline(None) is None and T.parse_baseline("none") is None and T.parse_baseline("None") is None
    assert T.parse_baseline("adjoint") == ("adjoint", 0)
    assert T.parse_baseline("cg-1") == ("cg", 1) and T.parse_baseline("cg-64") == ("cg", 64)
    for bad in ("cg", "cg-", "cg-0", "cg-65", "cg-4-2", "cg-a", "gridding", "", 4, True):
        with pytest.raises(ValueError):
            T.parse_baseline(bad)


def test_header_declares_the_two_entries():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^int (inr_adjoint\w*)\(", text, re.M))
    assert declared == {"inr_adjoint_nudft", "inr_adjoint_nudft_scratch"}
    assert int(re.search(r"^#define INR_ABI_VERSION (\d+)", text, re.M).group(1)) == L.ABI_VERSION == 7
    lib = L.load()
    for name in declared:
        assert name in L.SYMBOLS and hasattr(lib, name)


def test_argument_checks_need_no_gpu():
    lib = L.load()
    val, pos, w, out, scr = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 31, 1 << 32, 1 << 34))
    n = ctypes.c_int64(-1)
    C, H, W, M = 3, 40, 36, 257
    assert lib.inr_adjoint_nudft_scratch(C, H, W, M, ctypes.byref(n)) == 0
    need = n.value
    assert need == 2 * (64 + 64) * 320 == T.adjoint_scratch_floats(C, H, W, M)  # W, H and M to 64
    order = (("val", val), ("pos", pos), ("w", w), ("C", C), ("H", H), ("W", W), ("M", M), ("out", out), ("scr", scr),
             ("have", need), ("stream", None))
    call = lambda **kw: lib.inr_adjoint_nudft(*[kw.get(k, v) for k, v in order])
    for k in ("val", "pos", "out", "scr"):
        assert call(**{k: None}) == -1 and "null" in L.last_error()
    assert lib.inr_adjoint_nudft_scratch(C, H, W, M, None) == -1 and "null" in L.last_error()
    for bad in (0, 33):
        assert call(C=bad) == -1 and "1..32" in L.last_error()
        assert lib.inr_adjoint_nudft_scratch(bad, H, W, M, ctypes.byref(n)) == -1 and "1..32" in L.last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(H=1 << 16, W=1 << 15), dict(H=1 << 31, W=1),
               dict(H=1, W=(1 << 31) - 1)):
        assert call(**kw) == -1 and "H =" in L.last_error()
    for bad in (0, -5, 1 << 31):
        assert call(M=bad) == -1 and "M =" in L.last_error()
        assert lib.inr_adjoint_nudft_scratch(C, H, W, bad, ctypes.byref(n)) == -1
    for k, v in (("val", (1 << 20) + 4), ("pos", (1 << 30) + 4), ("out", (1 << 32) + 4), ("w", (1 << 31) + 2),
                 ("scr", (1 << 34) + 8)):
        assert call(**{k: ctypes.c_void_p(v)}) == -1 and "aligned" in L.last_error()
    assert call(have=need - 1) == -1 and "scratch" in L.last_error()
    assert call(out=val) == -1 and "overlaps val" in L.last_error()
    assert call(out=ctypes.c_void_p((1 << 20) + C * M * 8 - 8)) == -1 and "overlaps val" in L.last_error()  # last sample
    assert call(out=ctypes.c_void_p((1 << 30) + 16 * M - 16)) == -1 and "overlaps pos" in L.last_error()
    assert call(out=ctypes.c_void_p((1 << 31) + 1024)) == -1 and "overlaps w" in L.last_error()  # the last weight
    assert call(val=ctypes.c_void_p((1 << 32) - 8)) == -1 and "overlaps val" in L.last_error()  # val runs into out
    assert call(scr=ctypes.c_void_p((1 << 32) + 16)) == -1 and "scratch overlaps" in L.last_error()
    assert call(scr=ctypes.c_void_p((1 << 31) + 16)) == -1 and "scratch overlaps" in L.last_error()  # ... w
    assert call(w=None, scr=ctypes.c_void_p((1 << 20) + 16)) == -1 and "scratch overlaps" in L.last_error()  # ... val
    # a CPU tensor never falls back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.nudft_adjoint(torch.zeros(1, 3, 2), np.zeros((3, 2)), (6, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.cg_baseline(torch.zeros(3, 2), np.zeros((3, 2)), (1, 6, 5), None, 2)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=500, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


def test_trainers_refuse_before_any_device_call(tmp_path):
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    from inr_mi355x.trainer_base import ResidentFit, set_default_configs
    d = set_default_configs({})
    assert d["trajectory_baseline"] == "none" and d["trajectory_density"] is None
    image, coords, shape = make_kspace(2, 8, 8)
    pos_file = tmp_path / "p.npy"
    np.save(pos_file, T.spokes(8, 8, 2))
    cases = [dict(trajectory_baseline="cg-4"), dict(trajectory_baseline="adjoint", trajectory="none"),
             dict(trajectory_density="uniform"), dict(trajectory="spokes-4", trajectory_baseline="cg-0"),
             dict(trajectory="spokes-4", trajectory_baseline="cg-65"), dict(trajectory="spokes-4", trajectory_baseline="sense"),
             dict(trajectory="spokes-4", trajectory_baseline="cg-4", trajectory_density="voronoi"),
             dict(trajectory=str(pos_file), trajectory_baseline="cg-4", trajectory_density="ramp")]
    for kw in cases:
        with pytest.raises(ValueError, match="trajectory_baseline|trajectory_density"):
            INRTrainer(_cfg(**kw), image, coords, shape, "cuda:0")
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    with pytest.raises(ValueError, match="trajectory_baseline"):
        MultiscaleTrainer(_cfg(trajectory_baseline="cg-4"), image, coords, dist, None, shape, "cuda:0")
    with pytest.raises(ValueError, match="trajectory_baseline"):
        RingEnsembleTrainer(_cfg(trajectory_baseline="cg-4"), image, coords, shape, "cuda:0")
    with pytest.raises(NotImplementedError, match="trajectory"):
        MultiscaleTrainer(_cfg(trajectory="spokes-4", trajectory_baseline="cg-4"), image, coords, dist, None, shape, "cuda:0")
    with pytest.raises(NotImplementedError, match="trajectory"):
        RingEnsembleTrainer(_cfg(trajectory="spokes-4", trajectory_baseline="cg-4"), image, coords, shape, "cuda:0")
    # off: nothing is parsed beyond the two defaults; on: the weights are ready before any allocation
    fit = ResidentFit()
    fit._init_fit({}, (2, 8, 8), "cpu", 0, 0, 1, None)
    assert fit.trajectory_baseline is None and fit.trajectory_density is None and fit.gridding is None
    fit._init_fit({"trajectory": "spokes-4", "trajectory_baseline": "cg-3"}, (2, 8, 8), "cpu", 0, 0, 1, None,
                  trajectory_ok=True)
    assert fit.trajectory_baseline == ("cg", 3) and fit.trajectory_density[0] == "ramp"
    assert np.array_equal(fit.trajectory_density[1], T.density_ramp(4, 8, 8, 8)) and fit.gridding is None


def test_command_line_flags(tmp_path):
    from inr_mi355x.cli import parse_cli
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model: SIREN\nnormalization: max\n")
    opts, config = parse_cli(argv=["--config", str(cfg)])
    assert opts.trajectory_baseline is None and config["trajectory_baseline"] == "none"
    assert opts.trajectory_density is None and config["trajectory_density"] is None
    opts, config = parse_cli(argv=["--config", str(cfg), "--trajectory", "spokes-92", "--trajectory-baseline", "cg-10",
                                   "--trajectory-density", "uniform"])
    assert config["trajectory_baseline"] == "cg-10" and config["trajectory_density"] == "uniform"


@pytest.fixture(scope="module")
def cg_run():
    image, _, shape = make_kspace(2, 32, 32)
    C, H, W = shape
    img = torch.view_as_complex(ifft2c(image.reshape(C, H, W, 2).double()).contiguous()).numpy()
    pos = T.spokes(H, W, 12)
    y = T.nudft_numpy(img, pos)
    w = T.density_ramp(12, 32, H, W)
    return y, pos, shape, w, T.cg_baseline_numpy(y, pos, shape, w, 8)


def test_cg_objective_falls_geometrically(cg_run):
    y, pos, shape, w, (iterates, f) = cg_run
    C, H, W = shape
    assert len(iterates) == 8 and len(f) == 9 and iterates[0].shape == (C, H, W)
    assert f[0] == pytest.approx(float((w[None, :] * np.abs(y) ** 2).sum()), rel=1e-14)
    ratios = [f[i] / f[i + 1] for i in range(8)]
    print("objective ratios f_i / f_(i+1):", ", ".join("%.3f" % r for r in ratios))
    assert min(ratios) >= 1.5
    assert f[3] / f[4] >= 2.5
    # the objective carried along the recurrence is the objective of the iterate
    for k in (1, 4, 8):
        direct = float((w[None, :] * np.abs(T.nudft_numpy(iterates[k - 1], pos) - y) ** 2).sum())
        assert f[k] == pytest.approx(direct, rel=1e-9)


def test_cg_zero_iterations_is_the_weighted_adjoint(cg_run):
    y, pos, shape, w, _ = cg_run
    C, H, W = shape
    iterates, f = T.cg_baseline_numpy(y, pos, shape, w, 0)
    assert len(iterates) == 1 and len(f) == 1
    assert np.array_equal(iterates[0], T.nudft_adjoint_numpy(y, pos, H, W, w))
    assert f[0] == pytest.approx(float((w[None, :] * np.abs(T.nudft_numpy(iterates[0], pos) - y) ** 2).sum()), rel=1e-12)
