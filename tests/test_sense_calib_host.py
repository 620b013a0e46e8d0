"""SENSE fits on calibrated coil maps, host side: the settings and every refusal, the calibration block
and the ACS rule, the numpy restatements of csrc/inr_sense_calib.hip against their float64 statements, CG-SENSE in
float64, the checkpoint entry and its refusals, the header, the binding and the config file.

Criteria: 1e-12 relative where float64 is compared with float64; the project's 1e-5 relative L2 for fp32 text against
float64; bit equality where the same fp32 arithmetic sees the same inputs."""
import os
import re

import numpy as np
import pytest
import torch

import sense_calib_cases as CC
from conftest import ROOT

from inr_mi355x import _lib as L
from inr_mi355x import sense as S
from inr_mi355x import sense_calib as K

ENC = dict(embedding="gauss", scale=4, embedding_size=16, coordinates_size=3)


def rel_l2(got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _cx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1]


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_defaults_and_parsing():
    from inr_mi355x.train_sense import maps_settings, sense_settings
    assert maps_settings({"encoder": ENC}) is None and maps_settings({"encoder": ENC, "sense": {"maps": "learned"}}) is None
    d = maps_settings({"encoder": ENC, "sense": {"maps": "calibrated"}}, 640, 368)
    assert d == {"maps": "calibrated", "calib": {"size": [24, 24], "window": "hann", "floor": 0.0, "acs": True},
                 "baseline": None, "cg_lambda": 0.0}
    d = maps_settings({"sense": {"maps": "calibrated", "calib": {"size": [5, 64], "window": "none", "floor": 0.1,
                                                                 "acs": False},
                                 "baseline": "cg-7", "cg_lambda": 0.5, "coils_per_step": 2, "scale": 3.0}}, 12, 64)
    assert d["calib"] == {"size": [5, 64], "window": "none", "floor": 0.1, "acs": False}
    assert d["baseline"] == 7 and d["cg_lambda"] == 0.5
    assert maps_settings({"sense": {"maps": "calibrated", "baseline": "none"}})["baseline"] is None
    # the learned-maps settings do not change: the same five keys, coils_per_step defaulting to all coils in both modes
    base = sense_settings({"encoder": ENC}, n_coils=15)
    assert sense_settings({"encoder": ENC, "sense": {"maps": "learned"}}, n_coils=15) == base
    assert sense_settings({"encoder": ENC, "sense": {"maps": "calibrated"}}, n_coils=15)["coils_per_step"] == 15
    assert K.parse_sense_baseline("cg-1") == 1 and K.parse_sense_baseline("cg-64") == 64


@pytest.mark.parametrize("bad", [
    {"maps": "espirit"}, {"maps": "calibrated", "bogus": 1}, {"maps": "calibrated", "calib": {"sizes": [4, 4]}},
    {"maps": "calibrated", "calib": {"size": [1, 4]}}, {"maps": "calibrated", "calib": {"size": [4, 65]}},
    {"maps": "calibrated", "calib": {"size": [4]}}, {"maps": "calibrated", "calib": {"size": [4.5, 4]}},
    {"maps": "calibrated", "calib": {"size": [14, 4]}}, {"maps": "calibrated", "calib": {"size": [4, 12]}},
    {"maps": "calibrated", "calib": {"window": "hamming"}}, {"maps": "calibrated", "calib": {"floor": -0.1}},
    {"maps": "calibrated", "calib": {"floor": 1.0}}, {"maps": "calibrated", "calib": {"acs": 1}},
    {"maps": "calibrated", "calib": [4, 4]},
    {"maps": "calibrated", "baseline": "cg-0"}, {"maps": "calibrated", "baseline": "cg-65"},
    {"maps": "calibrated", "baseline": "adjoint"}, {"maps": "calibrated", "cg_lambda": -1.0},
    {"maps": "calibrated", "cg_lambda": float("nan")},
    {"maps": "calibrated", "net": {"network_width": 32}}, {"maps": "calibrated", "encoder": {"scale": 2}},
    {"maps": "calibrated", "max_stash_bytes": 1000},
    {"calib": {"size": [4, 4]}}, {"baseline": "cg-3"}, {"cg_lambda": 0.0}, {"maps": "learned", "baseline": "none"},
], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items())[:60])
def test_refusals(bad):
    from inr_mi355x.train_sense import maps_settings, sense_settings
    with pytest.raises(ValueError, match="sense"):
        maps_settings({"encoder": ENC, "sense": bad}, 12, 10)
    with pytest.raises(ValueError, match="sense"):  # ... and through the entry every trainer construction passes
        sense_settings({"encoder": ENC, "sense": bad}, n_coils=3)
        maps_settings({"encoder": ENC, "sense": bad}, 12, 10)


def test_block_and_acs_insertion():
    from inr_mi355x.train_sense import calibration_mask
    from inr_mi355x.undersampling import grid_mask
    C, H, W = 3, 12, 10
    assert K.block_range(12, 4) == (4, 8) and K.block_range(10, 4) == (3, 7) and K.block_range(9, 2) == (3, 5)
    assert K.block_range(7, 5) == (1, 6)  # rows H//2 - a//2 ... H//2 - a//2 + a - 1
    g = grid_mask(H, W, 3, 2).numpy() != 0
    blk = K.block_mask(H, W, 4, 4)
    assert blk.sum() == 16 and not g[blk].all()  # grid-3*2 keeps no centre
    calib = dict(K.CALIB_DEFAULTS, size=[4, 4])
    m, acc = calibration_mask(calib, "grid-3*2", (C, H, W))
    m = m.numpy().reshape(C, H, W)
    assert m.dtype == bool and all(np.array_equal(m[c], g | blk) for c in range(C))
    assert acc == (C * H * W) / m.sum() and 1.0 < acc < (H * W) / g.sum()
    # the caller's mask is used instead of the drawn one, per coil
    own = torch.zeros(C, H, W, dtype=torch.bool)
    own[1, 0, 0] = True
    m2 = calibration_mask(calib, "grid-3*2", (C, H, W), mask=own.reshape(-1))[0].numpy().reshape(C, H, W)
    assert m2.sum() == 3 * 16 + 1 and m2[1, 0, 0]
    # acs: false -- the block must be there already; the error names how many entries are not
    missing = int(C * (~g[blk]).sum())
    with pytest.raises(ValueError, match=rf"not fully sampled.*: {missing} of its {C * 16} entries"):
        calibration_mask(dict(calib, acs=False), "grid-3*2", (C, H, W))
    full, acc = calibration_mask(dict(calib, acs=False), "grid-3*2", (C, H, W), mask=torch.from_numpy(m.reshape(-1)))
    assert np.array_equal(full.numpy().reshape(C, H, W), m)
    assert calibration_mask(calib, None, (C, H, W)) == (None, 1.0)  # without any mask the block is taken as it is
    assert K.missing_in_block(g, 4, 4) == (~g[blk]).sum()


def test_window_and_cut_block():
    for a in (2, 3, 4, 5, 24, 64):
        w = K.window_1d(a, "hann")
        assert w[a // 2] == 1.0 and (w > 0).all() and w.max() == 1.0
        for k in range(1, a - a // 2):  # symmetric about the DC entry
            assert abs(w[a // 2 + k] - w[a // 2 - k]) <= 1e-15
        assert np.array_equal(K.window_1d(a, "none"), np.ones(a))
    k = CC.kspace(2, 9, 7)
    b = K.cut_block(k, 2, 2, "none")
    assert b.dtype == np.float32 and np.array_equal(b, k[:, 3:5, 2:4])
    bh = K.cut_block(torch.from_numpy(k), 5, 3, "hann")
    w = K.window_1d(5, "hann")[:, None] * K.window_1d(3, "hann")[None]
    assert np.array_equal(bh, (k[:, 2:7, 2:5].astype(np.float64) * w[None, :, :, None]).astype(np.float32))


# ---- the restatements --------------------------------------------------------------------------------------------------
def test_phasor_table_against_direct_exp():
    for N, a, n, win in ((12, 4, 12, (-1.0, 1.0)), (9, 2, 18, (-1.0, 1.0)), (132, 64, 7, (-0.5, 0.25)), (640, 24, 640, (-1, 1))):
        idx, pos = K.block_index(N, a), K.axis_positions(N, n, *win)
        want = np.exp(2j * np.pi * idx[:, None].astype(np.float64) * (pos[None, :] - N // 2) / N) / np.sqrt(N)
        got64 = K.phasor_table_float64(idx, pos, N)
        assert np.abs(got64 - want).max() <= 1e-12 / np.sqrt(N) * max(1.0, np.abs(idx).max())
        got = K.phasor_table(idx, pos, N)
        assert got.dtype == np.float32 and got.shape == (a, n, 2)
        assert np.array_equal(got, np.stack((got64.real, got64.imag), -1).astype(np.float32))
    assert np.array_equal(K.axis_positions(12, 12), np.arange(12.0))  # exact integers on the fit's own grid
    assert np.allclose(K.axis_positions(12, 24), np.arange(24) * 11 / 23)


@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.CASE_IDS)
def test_lowres_float64_is_the_zero_padded_ifft2c(case):
    (C, H, W), (a, b) = case
    for window in K.WINDOWS:
        block = K.cut_block(CC.kspace(C, H, W), a, b, window)
        pad = np.zeros((C, H, W), dtype=np.complex128)
        (r0, r1), (c0, c1) = K.block_range(H, a), K.block_range(W, b)
        pad[:, r0:r1, c0:c1] = _cx(block)
        want = S.fft2c_numpy(pad, inverse=True)
        ey = K.phasor_table_float64(K.block_index(H, a), K.axis_positions(H, H), H)
        ex = K.phasor_table_float64(K.block_index(W, b), K.axis_positions(W, W), W)
        assert rel_l2(K.lowres_float64(block, ey, ex), want) <= 1e-12


@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.CASE_IDS)
def test_fp32_restatements_against_float64(case):
    (C, H, W), (a, b) = case
    block = K.cut_block(CC.kspace(C, H, W), a, b, "hann")
    for Ho, Wo, window in ((H, W, K.FULL_WINDOW), (2 * H, 2 * W, K.FULL_WINDOW), (5, 7, (-0.5, 0.25, 0.1, 0.7))):
        ey, ex = K.grid_tables(H, W, a, b, Ho, Wo, window)
        low32 = K.lowres_numpy(block, ey, ex)
        ey64 = K.phasor_table_float64(K.block_index(H, a), K.axis_positions(H, Ho, *window[:2]), H)
        ex64 = K.phasor_table_float64(K.block_index(W, b), K.axis_positions(W, Wo, *window[2:]), W)
        low64 = K.lowres_float64(block, ey64, ex64)
        assert low32.dtype == np.float32 and low32.shape == (C, Ho, Wo, 2)
        assert rel_l2(_cx(low32), low64) <= 1e-5
        m32, r32 = K.maps_numpy(low32, C, Ho * Wo, 0.0)
        m64, r64 = K.maps_float64(low64, 0.0)
        assert rel_l2(_cx(m32).reshape(C, Ho, Wo), m64) <= 1e-5 and rel_l2(r32.reshape(Ho, Wo), r64) <= 1e-5
        got = K.calibrate_numpy(block, H, W, 0.0, Ho, Wo, window, fp32=True)
        assert np.array_equal(got[0], m32) and np.array_equal(got[1], r32)
        w64 = K.calibrate_numpy(block, H, W, 0.0, Ho, Wo, window)
        assert rel_l2(w64[0], m64) <= 1e-12


def test_maps_have_unit_rss_where_kept_and_are_zero_where_floored():
    (C, H, W), (a, b) = CC.KERNEL_CASES[0]
    block = K.cut_block(CC.kspace(C, H, W), a, b, "hann")
    low = K.lowres_numpy(block, *K.grid_tables(H, W, a, b))
    for floor in CC.FLOORS:
        maps, rss = K.maps_numpy(low, C, H * W, floor)
        keep = rss > np.float32(floor) * rss.max()
        assert (floor == 0.0 and keep.all()) or (floor > 0 and 0 < keep.sum() < keep.size)
        got = np.sqrt((maps.astype(np.float64) ** 2).sum(axis=(0, 2)))
        assert np.abs(got[keep] - 1.0).max() <= 4 * np.finfo(np.float32).eps * np.sqrt(C)
        assert (maps[:, ~keep] == 0).all()
        m64, r64 = K.maps_float64(_cx(low).reshape(C, H, W), floor)
        assert np.array_equal((r64 > floor * r64.max()).reshape(-1), keep)
        assert np.abs(np.sqrt((np.abs(m64) ** 2).sum(0)).reshape(-1)[keep] - 1).max() <= 1e-12
    z = np.zeros((2, 5, 2), np.float32)
    maps, rss = K.maps_numpy(z, 2, 5, 0.0)
    assert (maps == 0).all() and (rss == 0).all()  # r > 0 fails: zero, not NaN


@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.CASE_IDS)
def test_adjoint_text_is_the_dimg_of_the_grad_text(case):
    (G, H, W), _ = case
    sens, gx, img = CC.adjoint_inputs(G, H, W)
    for shift in (0, 1):
        want = S.sense_grad_numpy(img, sens, gx, G, H, W, CC.SCALE, shift)[0]
        got = K.sense_adjoint_numpy(sens, gx, G, H, W, CC.SCALE, shift)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    d64 = K.sense_adjoint_float64(sens, gx, G, H, W, CC.SCALE)
    assert rel_l2(_cx(K.sense_adjoint_numpy(sens, gx, G, H, W, CC.SCALE, 0)).reshape(H, W), d64) <= 1e-5


# ---- CG-SENSE ----------------------------------------------------------------------------------------------------------
def test_cg_full_sampling_unit_rss_is_done_after_one_iteration():
    """with every entry sampled and unit-RSS maps the normal operator is the identity: one iteration gives
    sum_c S_c^H x_c, x_c = ifft2c(y_c)"""
    maps, y, _, _ = CC.fit_problem()
    iterates, objective = K.cg_sense_numpy(maps, y, None, 1)
    want = np.sum(np.conj(maps) * S.fft2c_numpy(y, inverse=True), axis=0)
    # the maps are fp32 values: their RSS is 1 to fp32 rounding only, so is the operator; compare at that level ...
    assert rel_l2(iterates[0], want) <= 1e-6
    # ... and to 1e-12 once the maps are normalised in float64
    unit = maps / np.sqrt((np.abs(maps) ** 2).sum(0, keepdims=True))
    iterates, objective = K.cg_sense_numpy(unit, y, None, 1)
    want = np.sum(np.conj(unit) * S.fft2c_numpy(y, inverse=True), axis=0)
    assert rel_l2(iterates[0], want) <= 1e-12 and len(objective) == 2 and objective[1] < objective[0]


def test_cg_objective_does_not_increase_under_grid_plus_acs():
    maps, y, mask, _ = CC.fit_problem()
    assert 0 < mask.sum() < mask.size
    for lam in (0.0, 0.05):
        iterates, objective = K.cg_sense_numpy(maps, y, mask, 4, lam)
        assert len(iterates) == 4 and len(objective) == 5 and iterates[0].shape == CC.FIT_SHAPE[1:]
        assert all(b <= a * (1 + 1e-12) for a, b in zip(objective, objective[1:])), objective
        assert objective[-1] < objective[0]
        # the objective carried along equals the definition at the last iterate
        r = S.fft2c_numpy(maps * iterates[-1][None]) * mask - y * mask
        assert abs((np.abs(r) ** 2).sum() + lam * (np.abs(iterates[-1]) ** 2).sum() - objective[-1]) <= 1e-12 * objective[0]


def test_cg_fp32_operators_distance_is_the_recorded_one():
    """the figure the GPU test's bound is made from (sense_calib_cases.CG_FP32_REL_L2): measured here, on the host"""
    maps, y, mask, _ = CC.fit_problem()
    i64 = K.cg_sense_numpy(maps, y, mask, CC.CG_ITERS)[0]
    i32, o32 = K.cg_sense_numpy(maps, y, mask, CC.CG_ITERS, fp32=True)
    e = rel_l2(i32[-1].astype(np.complex128), i64[-1])
    print("fp32 numpy operators vs float64 after", CC.CG_ITERS, "iterations:", e)
    assert i32[-1].dtype == np.complex64 and 0 < e <= CC.CG_FP32_REL_L2
    assert 8 * CC.CG_FP32_REL_L2 < CC.CG_FLOOR_TOL  # so the GPU test's bound is the 1e-5 floor


# ---- checkpoints -------------------------------------------------------------------------------------------------------
def test_checkpoint_entry_and_refusals():
    block = torch.from_numpy(CC.fit_problem()[3])
    calib = dict(K.CALIB_DEFAULTS, size=[4, 4])
    st = K.calibrated_state(0.5, 3, calib, block)
    assert set(st) == {"scale", "coils_per_step", "maps", "calib", "block"} and st["maps"] == "calibrated"
    assert st["block"].data_ptr() != block.data_ptr() and torch.equal(st["block"], block)
    assert st["block"].numel() * 4 == 3 * 4 * 4 * 2 * 4 and 15 * 24 * 24 * 2 * 4 == 69120  # 69 KB at the brain shape
    net = K.image_net_state({"model.0.linear.weight": torch.ones(2, 3), "model.0.linear.bias": torch.zeros(2)})
    assert list(net) == ["image.model.0.linear.weight", "image.model.0.linear.bias"] and S.has_sense_keys(net)
    assert list(K.image_net_of(net)) == ["model.0.linear.weight", "model.0.linear.bias"]
    with pytest.raises(ValueError, match="image"):
        K.image_net_of(dict(net, **{"sens.model.0.weight": torch.zeros(1)}))
    K.check_calibrated_state(st, K.calibrated_state(0.5, 3, calib, block))
    for key, other in (("scale", K.calibrated_state(0.25, 3, calib, block)),
                       ("coils_per_step", K.calibrated_state(0.5, 2, calib, block)),
                       ("calib", K.calibrated_state(0.5, 3, dict(calib, window="none"), block)),
                       ("block", K.calibrated_state(0.5, 3, calib, block * 2)),
                       ("block", K.calibrated_state(0.5, 3, calib, block[:, :2]))):
        with pytest.raises(ValueError, match=key):
            K.check_calibrated_state(st, other)
    learned = {"scale": 0.5, "coils_per_step": 3, "enc_B": None, "net": {}, "encoder": {}}
    with pytest.raises(ValueError, match="maps = 'learned'"):
        K.check_calibrated_state(learned, st)
    with pytest.raises(ValueError, match="maps = 'calibrated'"):
        K.check_sense_mode(st, "learned")
    K.check_sense_mode(learned, "learned")  # learned-maps checkpoints carry no 'maps' entry and load as before


# ---- header, binding, build, command line ------------------------------------------------------------------------------
def test_header_binding_and_makefile():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_sense_lowres\(const float\* kc, const float\* ey, const float\* ex, int32_t C, int32_t a, "
                     r"int32_t b, int64_t Ho,\s+int64_t Wo, float\* out, void\* stream\);", text, re.M)
    assert re.search(r"^int inr_sense_maps\(const float\* low, int32_t C, int64_t P, float floor, float\* maps, "
                     r"float\* rss, void\* stream\);", text, re.M)
    assert re.search(r"^int inr_sense_adjoint\(const float\* sens, const float\* gx, int32_t G, int64_t H, int64_t W, "
                     r"float scale, int32_t shift,\s+float\* dimg, void\* stream\);", text, re.M)
    head = text[:text.index("#define INR_ABI_VERSION")]
    for name in ("inr_sense_lowres", "inr_sense_maps", "inr_sense_adjoint"):
        assert name in head[head.index("v7 additions"):]
        assert hasattr(L.load(), name)  # the built library exports it
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7 and L.load().inr_abi_version() == 7
    assert "#define INR_SENSE_CALIB_MAX 64\n" in text and L.SENSE_CALIB_MAX == 64
    assert [len(L.SYMBOLS[n][1]) for n in ("inr_sense_lowres", "inr_sense_maps", "inr_sense_adjoint")] == [10, 7, 9]
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        assert "inr_sense_calib.hip" in f.read()


def test_bindings_refuse_host_tensors_and_bad_shapes():
    kc, ey, ex = torch.zeros(2, 4, 4, 2), torch.zeros(4, 6, 2), torch.zeros(4, 5, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.sense_lowres(kc, ey, ex)
    with pytest.raises(RuntimeError, match="shape"):
        K.sense_lowres(kc, torch.zeros(3, 6, 2), ex)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.sense_maps(torch.zeros(2, 30, 2), 2, 30)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.sense_adjoint(torch.zeros(60, 2), torch.zeros(2, 6, 5, 2), 2, 6, 5, 1.0)
    with pytest.raises(RuntimeError, match="shape"):
        K.sense_adjoint(torch.zeros(60, 2), torch.zeros(2, 5, 6, 2), 2, 6, 5, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.cg_sense(torch.zeros(2, 30, 2), torch.zeros(60, 2), None, (2, 6, 5), 1)


def test_command_line_and_config():
    from inr_mi355x.cli import parse_cli
    from inr_mi355x.train_sense import add_sense_flags, apply_sense_flags, check_sense_config, maps_settings, sense_settings
    path = os.path.join(ROOT, "configs", "config_siren_sense_calibrated.yaml")
    opts, config = parse_cli(argv=["--config", path, "--synthetic", "15,640,368", "--max_steps", "3", "--val",
                                   "--save-images"], extra_flags=add_sense_flags)
    config = apply_sense_flags(config, opts)
    check_sense_config(config)
    assert config["undersampling"] == "grid-3*2" and sense_settings(config, n_coils=15)["coils_per_step"] == 15
    d = maps_settings(config, 640, 368)
    assert d == {"maps": "calibrated", "calib": dict(K.CALIB_DEFAULTS), "baseline": 10, "cg_lambda": 0.0}
    # the flags override the file; the learned-maps config becomes a calibrated one from the command line alone
    learned = os.path.join(ROOT, "configs", "config_siren_sense.yaml")
    opts, config = parse_cli(argv=["--config", learned, "--sense-maps", "calibrated", "--sense-baseline", "cg-4"],
                             extra_flags=add_sense_flags)
    config = apply_sense_flags(config, opts)
    assert config["sense"]["maps"] == "calibrated" and config["sense"]["baseline"] == "cg-4"
    with pytest.raises(ValueError, match="net"):  # ... but that file sizes a sensitivity network, which is refused
        maps_settings(config, 640, 368)
    opts, config = parse_cli(argv=["--config", path, "--sense-maps", "learned"], extra_flags=add_sense_flags)
    with pytest.raises(ValueError, match="calibrated"):
        maps_settings(apply_sense_flags(config, opts), 640, 368)
    opts, _ = parse_cli(argv=["--config", path])  # the other drivers' command lines do not have the flags
    assert not hasattr(opts, "sense_maps")
