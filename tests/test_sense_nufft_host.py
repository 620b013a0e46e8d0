"""Off-grid SENSE fits on calibrated maps, host side (no GPU): the fp32 numpy text of the two fused kernels
against the composition of the existing restatements, bit for bit; the float64 operators as conjugate transposes of each
other; refusals, keys and flags; the off-grid calibration's and the CG baseline's recorded distances."""
import numpy as np
import pytest

import sense_nufft_cases as NC


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def _cx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1]


def _prepare_text(x, H, W):
    """inr_nufft_prepare in fp32 numpy on coil images [G,H,W,2]: times 2 / (a_y a_x), centred in the zero grid"""
    from inr_mi355x import trajectory as T
    ay, ax = T.nufft_apodisation(H), T.nufft_apodisation(W)
    d = np.float32(2.0) / (ay[:, None] * ax[None, :])
    grid = np.zeros((x.shape[0], 2 * H, 2 * W, 2), dtype=np.float32)
    grid[:, H - H // 2:2 * H - H // 2, W - W // 2:2 * W - W // 2] = x * d[None, :, :, None]
    return grid


def _finish_text(grid, H, W):
    """inr_nufft_finish in fp32 numpy on a centred grid"""
    from inr_mi355x import trajectory as T
    ay, ax = T.nufft_apodisation(H), T.nufft_apodisation(W)
    d = np.float32(2.0) / (ay[:, None] * ax[None, :])
    return grid[:, H - H // 2:2 * H - H // 2, W - W // 2:2 * W - W // 2] * d[None, :, :, None]


@pytest.mark.parametrize("shape", NC.KERNEL_SHAPES, ids=NC.SHAPE_IDS)
def test_fp32_texts_equal_the_composition_of_the_existing_restatements(shape):
    from inr_mi355x import sense_nufft as SN
    from inr_mi355x.sense import sense_apply_numpy
    from inr_mi355x.sense_calib import sense_adjoint_numpy
    G, H, W = shape
    img, maps, grid, _, _ = NC.operands(G, H, W)
    got = SN.sense_nufft_prepare_numpy(img, maps, G, H, W, NC.SCALE)
    want = np.roll(_prepare_text(sense_apply_numpy(img, maps, G, H, W, NC.SCALE, 0), H, W), (H, W), (1, 2))
    assert _bits(got, want)
    assert np.count_nonzero(got) == G * H * W * 2  # the padding is zero, nothing else is
    got = SN.sense_nufft_finish_numpy(grid, maps, G, H, W, NC.SCALE)
    coil = np.ascontiguousarray(_finish_text(np.roll(grid, (H, W), (1, 2)), H, W))
    want = sense_adjoint_numpy(maps, coil, G, H, W, NC.SCALE, 0)
    assert _bits(got, want)
    old = NC.operands(G, H, W, seed=7)[0]
    assert _bits(SN.sense_nufft_finish_numpy(grid, maps, G, H, W, NC.SCALE, dimg=old), old + want)
    assert np.array_equal(SN.plain_roll(SN.plain_roll(grid, H, W), H, W), grid)


@pytest.mark.parametrize("shape", NC.KERNEL_SHAPES, ids=NC.SHAPE_IDS)
def test_adjoint_restatement_is_the_conjugate_transpose(shape):
    """<E x, y> = <x, E^H y> in float64, 1e-12 relative (weights folded into y)"""
    from inr_mi355x import sense_nufft as SN
    G, H, W = shape
    img, maps, _, val, w = NC.operands(G, H, W)
    pos = NC.positions(H, W)
    Ex = SN.sense_nufft_numpy(img, maps, pos, G, H, W, NC.SCALE)
    y = _cx(val)
    lhs = np.vdot(y * w[None, :], Ex)  # <W y, E x>
    EHy = SN.sense_nufft_adjoint_numpy(val, maps, pos, G, H, W, NC.SCALE, w)
    rhs = np.vdot(EHy, _cx(img.reshape(H, W, 2)))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_positions_cover_what_the_cases_promise():
    from inr_mi355x import trajectory as T
    for (_, H, W) in NC.KERNEL_SHAPES:
        pos = NC.positions(H, W)
        assert pos.shape == (NC.M, 2) and pos.dtype == np.float64
        jy, _ = T.nufft_taps(pos[:, 0], H)
        jx, _ = T.nufft_taps(pos[:, 1], W)
        assert (jy < 0).any() and (jy + 5 >= 2 * H).any() and (jx < 0).any() and (jx + 5 >= 2 * W).any()  # wrapping taps
        g = np.stack((np.floor(T._nufft_grid_position(pos[:, 0], H)), np.floor(T._nufft_grid_position(pos[:, 1], W))), 1)
        assert len({tuple(r) for r in g.tolist()}) < NC.M  # two samples in one cell
        assert (pos[:4] == np.round(pos[:4])).all()


# ---- refusals, keys and flags ----------------------------------------------------------------------------------------------
def _cfg(**over):
    from inr_mi355x.trainer_base import set_default_configs
    cfg = set_default_configs(dict(model="SIREN", net=dict(network_output_size=2), encoder=dict(embedding="gauss"),
                                   loss="L2"))
    cfg.update(over)
    return cfg


def test_calibrated_maps_accept_a_trajectory_and_learned_maps_do_not():
    from inr_mi355x.train_sense import check_sense_config, sense_operator
    check_sense_config(_cfg(trajectory="spokes-16", sense=dict(maps="calibrated")))
    check_sense_config(_cfg(trajectory="spokes-16-24", sense=dict(maps="calibrated", baseline="cg-3"),
                            trajectory_operator="exact", trajectory_density="uniform"))
    for sense in (None, {}, dict(maps="learned"), dict(net=dict(network_width=32))):
        with pytest.raises(NotImplementedError, match="trajectory"):
            check_sense_config(_cfg(trajectory="spokes-16", sense=sense))
    assert sense_operator(_cfg(sense=dict(maps="calibrated"))) is None
    assert sense_operator(_cfg(trajectory="spokes-16", sense=dict(maps="calibrated"))) == "gridding"  # the default HERE
    assert sense_operator(_cfg(trajectory="spokes-16", trajectory_operator="exact")) == "exact"
    with pytest.raises(ValueError, match="trajectory_operator"):
        sense_operator(_cfg(trajectory="spokes-16", trajectory_operator="fast"))


@pytest.mark.parametrize("over,sense,match", [
    (dict(undersampling="grid-3*2"), {}, "IS the sampling"),
    ({}, dict(calib=dict(acs=True)), "acs"),
    ({}, dict(calib=dict(acs=False)), "acs"),
    (dict(trajectory_baseline="cg-3"), {}, "trajectory_baseline"),
    (dict(loss="HDR"), {}, "HDR"),
])
def test_what_an_offgrid_sense_fit_refuses(over, sense, match):
    from inr_mi355x.train_sense import check_offgrid_sense_config, check_sense_config
    cfg = _cfg(trajectory="spokes-16", sense=dict(dict(maps="calibrated"), **sense), **over)
    with pytest.raises((ValueError, NotImplementedError), match=match):
        check_sense_config(cfg)
    with pytest.raises(ValueError, match="IS the sampling"):
        check_offgrid_sense_config(_cfg(trajectory="spokes-16", sense=dict(maps="calibrated")), mask=np.ones(4))


def test_cli_flags_reach_the_config(tmp_path):
    import yaml
    from inr_mi355x.cli import parse_cli
    from inr_mi355x.train_sense import add_sense_flags, apply_sense_flags, check_sense_config, sense_operator
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(dict(model="SIREN", net=dict(network_output_size=2), encoder=dict(embedding="gauss"),
                                        loss="L2")))
    import sys
    argv, sys.argv = sys.argv, ["train_sense", "--config", str(path), "--trajectory", "spokes-8", "--trajectory-operator",
                                "exact", "--trajectory-density", "uniform", "--sense-maps", "calibrated",
                                "--sense-baseline", "cg-2"]
    try:
        opts, config = parse_cli(extra_flags=add_sense_flags)
    finally:
        sys.argv = argv
    config = apply_sense_flags(config, opts)
    assert config["trajectory"] == "spokes-8" and config["trajectory_density"] == "uniform"
    assert config["sense"] == dict(maps="calibrated", baseline="cg-2") and sense_operator(config) == "exact"
    check_sense_config(config)


def test_shipped_config_is_an_offgrid_calibrated_fit():
    import os
    import yaml
    from inr_mi355x.train_sense import check_sense_config, maps_settings, sense_operator
    from inr_mi355x.trainer_base import set_default_configs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "config_siren_sense_radial.yaml")) as f:
        cfg = set_default_configs(yaml.safe_load(f))
    check_sense_config(cfg)
    assert sense_operator(cfg) == "gridding" and maps_settings(cfg)["maps"] == "calibrated"
    assert cfg["trajectory"].startswith("spokes-")


# ---- recorded distances ------------------------------------------------------------------------------------------------------
def test_offgrid_calibration_distance_is_the_recorded_one():
    """maps from the samples alone (density-weighted exact adjoint -> fft2c -> block -> calibrate) against maps from the
    Cartesian centre of the same scan: the recorded relative L2 distance is reproduced; both have unit RSS where kept"""
    from inr_mi355x import sense_calib as K
    from inr_mi355x import trajectory as T
    from inr_mi355x.sense import fft2c_numpy
    from inr_mi355x.synthetic import make_kspace
    C, H, W = NC.CALIB_SHAPE
    k = make_kspace(C, H, W)[0].reshape(C, H, W, 2).numpy()
    parsed = T.parse_trajectory(NC.CALIB_TRAJECTORY)
    pos = T.positions(parsed, H, W)
    name, w = T.parse_density(None, parsed, H, W)
    assert name == "ramp" and abs(w.sum() - H * W) <= 1e-9 * H * W
    y = T.nudft_numpy(fft2c_numpy(_cx(k), inverse=True), pos)
    back = fft2c_numpy(T.nudft_adjoint_numpy(y, pos, H, W, w))
    off = K.cut_block(np.stack((back.real, back.imag), -1), *NC.CALIB_BLOCK, "hann")
    cart = K.cut_block(k, *NC.CALIB_BLOCK, "hann")
    m_off, rss_off = K.calibrate_numpy(off, H, W)
    m_cart, rss_cart = K.calibrate_numpy(cart, H, W)
    for m, rss in ((m_off, rss_off), (m_cart, rss_cart)):
        kept = rss > 0
        assert kept.any() and np.allclose(np.sqrt((np.abs(m) ** 2).sum(axis=0))[kept], 1.0, rtol=0, atol=1e-12)
    dist = float(np.linalg.norm(m_off - m_cart) / np.linalg.norm(m_cart))
    print(f"off-grid calibration: relative L2 distance of the maps from the Cartesian-centre maps {dist:.4e}")
    assert abs(dist - NC.CALIB_REL_L2) <= 0.02 * NC.CALIB_REL_L2, (dist, NC.CALIB_REL_L2)


def test_cg_fp32_operators_distance_is_the_recorded_one():
    from inr_mi355x import sense_nufft as SN
    maps, y, pos, w, _ = NC.fit_samples()
    want, obj64 = SN.cg_sense_nufft_numpy(maps, y, pos, w, NC.CG_ITERS)
    got, obj32 = SN.cg_sense_nufft_numpy(maps, y, pos, w, NC.CG_ITERS, fp32=True)
    errs = [float(np.linalg.norm(g - x) / np.linalg.norm(x)) for g, x in zip(got, want)]
    print("non-Cartesian CG-SENSE, fp32 operators vs float64, per iteration:", errs, "objective", obj64)
    assert all(b <= a for a, b in zip(obj64, obj64[1:])), obj64
    assert 0.5 * NC.CG_FP32_REL_L2 <= errs[-1] <= 1.05 * NC.CG_FP32_REL_L2, (errs, NC.CG_FP32_REL_L2)
