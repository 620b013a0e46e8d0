"""Off-grid fits on the host (inr_mi355x/trajectory.py): the fp64 definition against the centred
FFT, the spoke geometry, the switch's grammar, the coordinates of a trajectory, the library's argument checks on fake
pointers and the trainers' refusals.  None of it touches a GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import trajectory as T
from inr_mi355x.evalchain import fft2c
from inr_mi355x.synthetic import create_coords, make_kspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_positions(H, W):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([yy.ravel(), xx.ravel()], axis=1)


def _random_image(C, H, W, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((C, H, W)) + 1j * g.standard_normal((C, H, W))


@pytest.mark.parametrize("H,W", [(6, 5), (7, 8), (5, 7)])
def test_definition_is_the_centred_fft_at_integer_positions(H, W):
    img = _random_image(2, H, W, seed=H * 10 + W)
    pairs = torch.from_numpy(np.stack([img.real, img.imag], -1))  # float64 pairs
    want = torch.view_as_complex(fft2c(pairs)).numpy().reshape(2, -1)
    pos = _grid_positions(H, W)
    got = T.nudft_numpy(img, pos)
    assert got.dtype == np.complex128 and got.shape == (2, H * W)
    assert np.abs(got - want).max() <= 1e-12
    # periodic in both axes
    for shift in ((H, 0), (0, W), (-2 * H, 3 * W)):
        assert np.abs(T.nudft_numpy(img, pos + np.array(shift, dtype=np.float64)) - want).max() <= 1e-12


def test_delta_image_gives_a_phasor():
    H, W = 6, 5
    img = np.zeros((1, H, W), dtype=np.complex128)
    img[0, 1, 3] = 1.0
    pos = np.array([[2.5, 0.25], [0.0, 4.0], [-3.5, 7.75]])
    got = T.nudft_numpy(img, pos)[0]
    want = np.exp(-2j * np.pi * ((pos[:, 0] - 3) * (1 - 3) / H + (pos[:, 1] - 2) * (3 - 2) / W)) / math.sqrt(H * W)
    assert np.abs(got - want).max() <= 1e-14


@pytest.mark.parametrize("H,W,R", [(32, 32, None), (7, 8, None), (40, 36, 17), (5, 7, 64)])
def test_spokes_geometry(H, W, R):
    n = 9
    pos = T.spokes(H, W, n, R)
    R = R or max(H, W)
    assert pos.dtype == np.float64 and pos.shape == (n * R, 2)
    assert pos[:, 0].min() >= 0 and pos[:, 0].max() <= H - 1 and pos[:, 1].min() >= 0 and pos[:, 1].max() <= W - 1
    sp = pos.reshape(n, R, 2)
    assert np.array_equal(sp[:, R // 2, 0], np.full(n, H // 2)) and np.array_equal(sp[:, R // 2, 1], np.full(n, W // 2))
    # the angle of a spoke from its first sample (rho = -1): (u - c) / a = -(sin, cos)
    cy, cx = H // 2, W // 2
    ay, ax = min(cy, H - 1 - cy), min(cx, W - 1 - cx)
    theta = np.arctan2(-(sp[:, 0, 0] - cy) / ay, -(sp[:, 0, 1] - cx) / ax)
    step = np.angle(np.exp(1j * np.diff(theta)))
    golden = math.pi * (math.sqrt(5.0) - 1.0) / 2.0
    assert T.GOLDEN_ANGLE == golden
    assert np.abs(step - np.angle(np.exp(1j * golden))).max() <= 1e-12
    assert abs(np.angle(np.exp(1j * theta[0]))) <= 1e-12  # spoke 0 lies along x
    # `first` shifts the sequence
    assert np.array_equal(T.spokes(H, W, n - 3, R, first=3), pos[3 * R:])
    for bad in ((0, 5, 3), (5, 5, 0)):
        with pytest.raises(ValueError):
            T.spokes(*bad)


def test_parse_trajectory_grammar(tmp_path):
    assert T.parse_trajectory(None) is None and T.parse_trajectory("none") is None and T.parse_trajectory("None") is None
    assert T.parse_trajectory("spokes-24") == ("spokes", 24, None)
    assert T.parse_trajectory("spokes-92-640") == ("spokes", 92, 640)
    for bad in ("spokes", "spokes-", "spokes-0", "spokes-3-1", "spokes-a", "spokes-3-4-5", "radial-4", "", 7, 2.5,
                str(tmp_path / "missing.npy"), "positions.txt"):
        with pytest.raises(ValueError):
            T.parse_trajectory(bad)
    pos = T.spokes(8, 6, 2)
    good = tmp_path / "p.npy"
    np.save(good, pos)
    kind, path, back = T.parse_trajectory(str(good))
    assert kind == "file" and path == str(good) and np.array_equal(back, pos)
    for name, arr in (("nan", np.where(np.arange(pos.size).reshape(pos.shape) == 3, np.nan, pos)),
                      ("inf", np.where(np.arange(pos.size).reshape(pos.shape) == 0, np.inf, pos)),
                      ("f32", pos.astype(np.float32)), ("flat", pos.ravel()), ("cols", np.zeros((4, 3))),
                      ("empty", np.zeros((0, 2)))):
        f = tmp_path / (name + ".npy")
        np.save(f, arr)
        with pytest.raises(ValueError):
            T.parse_trajectory(str(f))
    d = T.describe(T.parse_trajectory("spokes-24"), 32, 32)
    assert d == {"kind": "spokes", "spokes": 24, "readout": 32, "rows_per_coil": 768, "acceleration": 1024 / 768}
    d = T.describe(T.parse_trajectory("spokes-3-10"), 8, 6)
    assert d["readout"] == 10 and d["rows_per_coil"] == 30 and d["acceleration"] == 48 / 30
    d = T.describe(T.parse_trajectory(str(good)), 8, 6)
    assert d == {"kind": "file", "spokes": None, "readout": None, "rows_per_coil": 16, "acceleration": 3.0}
    assert T.describe(None, 8, 6) is None


@pytest.mark.parametrize("C,H,W", [(1, 6, 5), (3, 7, 8), (15, 64, 48)])
def test_trajectory_coords_of_the_grid_is_create_coords(C, H, W):
    got = T.trajectory_coords(_grid_positions(H, W), C, H, W)
    want = create_coords(C, H, W)
    assert got.dtype == torch.float32 and got.shape == want.shape == (C * H * W, 3)
    # One ulp of the axis, 2^-23 (the spacing of fp32 at its ends +-1).  torch.linspace forms a + i * step in fp32, so its
    # own values near 0 are off the exact ones by up to half of that -- many ulps OF THOSE VALUES -- while the fp64-formed
    # rows are the correctly rounded ones: the two cannot agree more closely than in units of the axis.
    diff = np.abs(got.numpy().astype(np.float64) - want.numpy().astype(np.float64))
    print("max |trajectory_coords - create_coords| = %.3f ulp(1)" % (diff.max() / 2.0 ** -23))
    assert diff.max() <= 2.0 ** -23
    # coil-major, and fp64-formed off the grid
    pos = np.array([[0.5, 1.25], [H - 1.0, 0.0]])
    rows = T.trajectory_coords(pos, C, H, W).numpy().reshape(C, 2, 3)
    assert np.array_equal(rows[:, 0, 1], np.full(C, np.float32(-1.0 + 2.0 * 0.5 / (H - 1))))
    assert np.array_equal(rows[:, 0, 2], np.full(C, np.float32(-1.0 + 2.0 * 1.25 / (W - 1))))
    assert np.array_equal(rows[:, 1, 1], np.ones(C, np.float32)) and np.array_equal(rows[:, 1, 2], -np.ones(C, np.float32))
    assert np.array_equal(rows[:, 0, 0], rows[:, 1, 0]) and rows[0, 0, 0] == -1.0


def test_header_declares_the_two_entries():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^int (inr_nudft\w*)\(", text, re.M))
    assert declared == {"inr_nudft", "inr_nudft_scratch"}
    assert int(re.search(r"^#define INR_NUDFT_TILE (\d+)", text, re.M).group(1)) == L.NUDFT_TILE
    assert int(re.search(r"^#define INR_ABI_VERSION (\d+)", text, re.M).group(1)) == L.ABI_VERSION == 7
    lib = L.load()
    for name in declared:
        assert name in L.SYMBOLS and hasattr(lib, name)


def test_argument_checks_need_no_gpu():
    lib = L.load()
    img, pos, out, scr = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 32, 1 << 34))
    n = ctypes.c_int64(-1)
    C, H, W, M = 3, 40, 36, 257
    assert lib.inr_nudft_scratch(C, H, W, M, ctypes.byref(n)) == 0
    need = n.value
    assert need == 2 * (48 + 64) * 320 == T.scratch_floats(C, H, W, M)  # W to 16, H to 64, M to 64
    call = lambda **kw: lib.inr_nudft(*[kw.get(k, v) for k, v in (("img", img), ("C", C), ("H", H), ("W", W), ("pos", pos),
                                                                    ("M", M), ("out", out), ("scr", scr), ("have", need),
                                                                    ("stream", None))])
    for k in ("img", "pos", "out", "scr"):
        assert call(**{k: None}) == -1 and "null" in L.last_error()
    assert lib.inr_nudft_scratch(C, H, W, M, None) == -1 and "null" in L.last_error()
    for bad in (0, 33):
        assert call(C=bad) == -1 and "1..32" in L.last_error()
        assert lib.inr_nudft_scratch(bad, H, W, M, ctypes.byref(n)) == -1 and "1..32" in L.last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(H=1 << 16, W=1 << 15), dict(H=1 << 31, W=1)):
        assert call(**kw) == -1 and "H =" in L.last_error()
    for bad in (0, -5, 1 << 31):
        assert call(M=bad) == -1 and "M =" in L.last_error()
        assert lib.inr_nudft_scratch(C, H, W, bad, ctypes.byref(n)) == -1
    for k, v in (("img", (1 << 20) + 4), ("pos", (1 << 30) + 4), ("out", (1 << 32) + 4), ("scr", (1 << 34) + 8)):
        assert call(**{k: ctypes.c_void_p(v)}) == -1 and "aligned" in L.last_error()
    assert call(have=need - 1) == -1 and "scratch" in L.last_error()
    assert call(out=img) == -1 and "overlaps img" in L.last_error()
    assert call(out=ctypes.c_void_p((1 << 20) + C * H * W * 8 - 8)) == -1 and "overlaps img" in L.last_error()  # last pixel
    assert call(out=ctypes.c_void_p((1 << 30) + 16 * M - 16)) == -1 and "overlaps pos" in L.last_error()
    assert call(scr=ctypes.c_void_p((1 << 32) + 16)) == -1 and "scratch overlaps" in L.last_error()
    # a CPU tensor never falls back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.nudft(torch.zeros(1, 6, 5, 2), np.zeros((1, 2)))


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=500, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               trajectory="spokes-4")
    cfg.update(kw)
    return cfg


    def __getattr__(self, name):
        raise AssertionError("the constructor reached the device")


def test_trainers_refuse_before_any_device_call():
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    from inr_mi355x.trainer_base import ResidentFit, set_default_configs
    assert set_default_configs({})["trajectory"] == "none"
    image, coords, shape = make_kspace(2, 8, 8)
    mask = torch.ones(2 * 8 * 8, 1, dtype=torch.bool)
    cases = [(dict(transform=True), {}, ValueError), (dict(undersampling="radial-4"), {}, ValueError),
             (dict(undersampling="grid-2*2"), {}, ValueError), ({}, dict(mask=mask), ValueError),
             (dict(per_coil=True), {}, ValueError), (dict(use_tv=True), {}, ValueError),
             (dict(loss="LSL"), {}, NotImplementedError), ({}, dict(graph_steps=True), NotImplementedError),
             ({}, dict(world=2, rank=0), NotImplementedError), (dict(trajectory="spirals-3"), {}, ValueError)]
    for cfg_kw, ctor_kw, exc in cases:
        with pytest.raises(exc, match="trajectory"):
            INRTrainer(_cfg(**cfg_kw), image, coords, shape, "cuda:0", **ctor_kw)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    with pytest.raises(NotImplementedError, match="trajectory"):
        MultiscaleTrainer(_cfg(), image, coords, dist, None, shape, "cuda:0")
    with pytest.raises(NotImplementedError, match="trajectory"):
        RingEnsembleTrainer(_cfg(), image, coords, shape, "cuda:0")
    # off: the key is "none" and nothing is parsed
    fit = ResidentFit()
    fit._init_fit({}, (2, 8, 8), "cpu", 0, 0, 1, None)
    assert fit.trajectory is None and fit.trajectory_info is None and fit.config["trajectory"] == "none"
    fit._init_fit({"trajectory": "spokes-4"}, (2, 8, 8), "cpu", 0, 0, 1, None, trajectory_ok=True)
    assert fit.trajectory == ("spokes", 4, None) and fit.trajectory_info["rows_per_coil"] == 32


def test_command_line_flag(tmp_path):
    from inr_mi355x.cli import parse_cli
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model: SIREN\nnormalization: max\n")
    opts, config = parse_cli(argv=["--config", str(cfg)])
    assert opts.trajectory is None and config["trajectory"] == "none"
    opts, config = parse_cli(argv=["--config", str(cfg), "--trajectory", "spokes-92"])
    assert config["trajectory"] == "spokes-92"
