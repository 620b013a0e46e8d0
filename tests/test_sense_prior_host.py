"""The total-variation prior on the image of a SENSE fit, host side: the fp32 numpy text of
csrc/inr_image_tv.hip against its float64 statement, that statement against torch's float64 autograd, eps = 0, the
accumulating form, the settings and every refusal, the command line, the header, the binding and the Makefile.

Criteria -- none of them new: 1e-5 relative (L2 for arrays) for fp32 text against float64; 1e-12 where float64 is compared
with float64; bit equality where the same fp32 arithmetic sees the same inputs."""
import os
import re

import numpy as np
import pytest
import torch

import sense_prior_cases as PC
from conftest import ROOT

from inr_mi355x import _lib as L
from inr_mi355x import sense_prior as P

ENC = dict(embedding="gauss", scale=4, embedding_size=16, coordinates_size=3)


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.abs(got).max(initial=0.0))


# ---- the text ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)
def test_fp32_text_against_float64(case):
    (H, W), eps = case
    img = PC.image(H, W, eps)
    v, g = P.image_tv_numpy(img, H, W, PC.WEIGHT, eps)
    v64, g64 = P.image_tv_float64(img, H, W, PC.WEIGHT, eps)
    assert v.dtype == np.float32 and g.dtype == np.float32 and g.shape == (H * W, 2)
    ev = abs(float(v) - v64) / abs(v64) if v64 != 0 else abs(float(v))
    eg = rel_l2(g, g64)
    print(case, "fp32 text vs float64: value", ev, "gradient", eg)
    assert ev <= 1e-5 and eg <= 1e-5
    # the value is the fp64 sum of the text's fp32 terms, scaled in fp64, rounded once
    terms = P.image_tv_terms(img, H, W, eps)
    assert terms.dtype == np.float32 and terms.shape == (H, W)
    assert v == np.float32(terms.astype(np.float64).sum() * (np.float64(np.float32(PC.WEIGHT)) / (H * W)))


SMOOTH = [(i, c) for i, c in zip(PC.CASE_IDS, PC.CASES) if c[1] > 0]


@pytest.mark.parametrize("case", [c for _, c in SMOOTH], ids=[i for i, _ in SMOOTH])
def test_float64_statement_against_autograd(case):
    (H, W), eps = case
    img = PC.image(H, W, eps)
    t = torch.from_numpy(img.astype(np.float64)).reshape(H, W, 2).requires_grad_(True)
    value = PC.tv_torch(torch.view_as_complex(t), PC.WEIGHT, eps)
    value.backward()
    v64, g64 = P.image_tv_float64(img, H, W, PC.WEIGHT, eps)
    assert abs(v64 - float(value.detach())) <= 1e-12 * abs(float(value.detach()))
    assert rel_l2(g64, t.grad.reshape(H * W, 2).numpy()) <= 1e-12


@pytest.mark.parametrize("shape", PC.SHAPES + (PC.LARGE,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_eps_zero_with_a_flat_patch(shape):
    H, W = shape
    img = PC.image(H, W, 0.0)
    zero = PC.zero_n(H, W)
    assert zero.sum() >= 1 and np.array_equal(P.image_tv_terms(img, H, W, 0.0) == 0, zero)  # n = 0 exactly there
    v, g = P.image_tv_numpy(img, H, W, PC.WEIGHT, 0.0)
    v64, g64 = P.image_tv_float64(img, H, W, PC.WEIGHT, 0.0)
    assert np.isfinite(v) and np.isfinite(g).all() and np.isfinite(v64) and np.isfinite(g64).all()
    still = PC.zero_grad(H, W).reshape(-1)
    assert still.sum() >= 1 and not g[still].any() and not g64[still].any()
    # a constant image: value 0 and gradient 0, for eps = 0 and eps > 0
    flat = np.tile(np.float32([0.25, -0.5]), (H * W, 1))
    for eps in (0.0, 1e-3):
        v, g = P.image_tv_numpy(flat, H, W, PC.WEIGHT, eps)
        assert v == 0 and not g.any()
        v64, g64 = P.image_tv_float64(flat, H, W, PC.WEIGHT, eps)
        assert v64 == 0 and not g64.any()


@pytest.mark.parametrize("case", PC.CASES[:6] + PC.CASES[-3:], ids=PC.CASE_IDS[:6] + PC.CASE_IDS[-3:])
def test_accumulate_is_one_fp32_add(case):
    (H, W), eps = case
    img, d0 = PC.image(H, W, eps), PC.dimg0(H, W)
    v, g = P.image_tv_numpy(img, H, W, PC.WEIGHT, eps)
    keep = d0.copy()
    va, ga = P.image_tv_numpy(img, H, W, PC.WEIGHT, eps, accumulate=True, dimg=d0)
    assert va == v and np.array_equal(d0, keep)  # the input is left alone
    assert ga.dtype == np.float32 and np.array_equal(ga.view(np.int32), (d0 + g).view(np.int32))
    with pytest.raises(ValueError, match="dimg"):
        P.image_tv_numpy(img, H, W, PC.WEIGHT, eps, accumulate=True)


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_parse_prior_defaults():
    assert P.parse_prior(None) is None and P.parse_prior("none") is None and P.parse_prior("None") is None
    assert P.parse_prior({}) is None and P.parse_prior({"kind": "none"}) is None
    assert P.parse_prior({"weight": 1e-3}) == {"kind": "tv", "weight": 1e-3, "eps": 1e-3}
    assert P.parse_prior({"kind": "tv", "weight": 2, "eps": 0}) == {"kind": "tv", "weight": 2.0, "eps": 0.0}
    assert P.parse_prior({"kind": "tv", "weight": "1e-2", "eps": 1e-4}) == {"kind": "tv", "weight": 1e-2, "eps": 1e-4}
    assert P.PRIOR_EPS == 1e-3


@pytest.mark.parametrize("bad", [
    {"kind": "tv"}, {"eps": 1e-3}, {"kind": "l1", "weight": 1.0}, {"kind": "tv", "weight": 1.0, "bogus": 1},
    {"weight": 0.0}, {"weight": -1.0}, {"weight": float("nan")}, {"weight": float("inf")}, {"weight": "much"},
    {"weight": True}, {"weight": 1.0, "eps": -1e-3}, {"weight": 1.0, "eps": float("nan")},
    {"weight": 1.0, "eps": float("inf")}, {"weight": 1.0, "eps": None}, "tv", 3, ["tv", 1.0],
], ids=repr)
def test_parse_prior_refusals(bad):
    with pytest.raises(ValueError, match="prior"):
        P.parse_prior(bad)


def test_trainer_settings_admit_the_key_and_leave_the_others_alone():
    from inr_mi355x import train_sense as T
    assert T.PRIOR_KEYS == ("prior",) and "prior" not in T.SENSE_KEYS and "prior" not in T.MAPS_KEYS
    assert T.SENSE_KEYS == ("coils_per_step", "scale", "net", "encoder", "max_stash_bytes")
    assert T.MAPS_KEYS == ("maps", "calib", "baseline", "cg_lambda")
    prior = {"weight": 1e-3}
    for sense in ({}, {"maps": "learned"}, {"maps": "calibrated"}):
        cfg, cfg_p = {"encoder": ENC, "sense": dict(sense)}, {"encoder": ENC, "sense": dict(sense, prior=prior)}
        assert T.prior_settings(cfg) is None and T.prior_settings({"encoder": ENC}) is None
        assert T.prior_settings(cfg_p) == {"kind": "tv", "weight": 1e-3, "eps": 1e-3}
        assert T.prior_settings({"encoder": ENC, "sense": dict(sense, prior="none")}) is None
        assert T.sense_settings(cfg_p, n_coils=15) == T.sense_settings(cfg, n_coils=15)  # the same dictionaries
        assert T.maps_settings(cfg_p, 64, 64) == T.maps_settings(cfg, 64, 64)
    with pytest.raises(ValueError, match="prior"):
        T.prior_settings({"sense": {"prior": {"kind": "tv"}}})
    with pytest.raises(ValueError, match="bogus"):
        T.prior_settings({"sense": {"bogus": 1}})


def test_use_tv_stays_refused_and_points_at_the_key():
    from inr_mi355x.train_sense import check_sense_config
    from inr_mi355x.trainer_base import set_default_configs
    cfg = set_default_configs(dict(model="SIREN", loss="L2", encoder=ENC, net={}, use_tv=True,
                                   sense={"prior": {"weight": 1e-3}}))
    with pytest.raises(NotImplementedError) as err:
        check_sense_config(cfg)
    assert "use_tv" in str(err.value) and "sense.prior" in str(err.value)
    cfg["use_tv"] = False
    check_sense_config(cfg)  # the prior itself is admitted


def test_command_line_and_config():
    from inr_mi355x.cli import parse_cli
    from inr_mi355x.train_sense import add_sense_flags, apply_sense_flags, check_sense_config, maps_settings, prior_settings
    plain = os.path.join(ROOT, "configs", "config_siren_sense_calibrated.yaml")
    opts, config = parse_cli(argv=["--config", plain, "--sense-prior", "tv:1e-3:1e-4"], extra_flags=add_sense_flags)
    config = apply_sense_flags(config, opts)
    assert config["sense"]["prior"] == {"kind": "tv", "weight": 1e-3, "eps": 1e-4}
    assert prior_settings(config) == {"kind": "tv", "weight": 1e-3, "eps": 1e-4}
    check_sense_config(config)
    opts, config = parse_cli(argv=["--config", plain, "--sense-prior", "tv:0.5"], extra_flags=add_sense_flags)
    assert prior_settings(apply_sense_flags(config, opts)) == {"kind": "tv", "weight": 0.5, "eps": 1e-3}
    opts, config = parse_cli(argv=["--config", plain], extra_flags=add_sense_flags)
    assert "prior" not in apply_sense_flags(config, opts)["sense"] and prior_settings(config) is None
    # the config file carries the key; `none` on the command line switches it off; learned maps take the flag too
    path = os.path.join(ROOT, "configs", "config_siren_sense_calibrated_tv.yaml")
    opts, config = parse_cli(argv=["--config", path], extra_flags=add_sense_flags)
    config = apply_sense_flags(config, opts)
    check_sense_config(config)
    assert prior_settings(config) == {"kind": "tv", "weight": 1e-4, "eps": 1e-3}
    opts, base = parse_cli(argv=["--config", plain], extra_flags=add_sense_flags)
    assert maps_settings(config, 640, 368) == maps_settings(base, 640, 368)
    assert {k: v for k, v in config.items() if k != "sense"} == {k: v for k, v in base.items() if k != "sense"}
    opts, config = parse_cli(argv=["--config", path, "--sense-prior", "none"], extra_flags=add_sense_flags)
    assert prior_settings(apply_sense_flags(config, opts)) is None
    learned = os.path.join(ROOT, "configs", "config_siren_sense.yaml")
    opts, config = parse_cli(argv=["--config", learned, "--sense-prior", "tv:2e-4"], extra_flags=add_sense_flags)
    config = apply_sense_flags(config, opts)
    assert prior_settings(config)["weight"] == 2e-4 and maps_settings(config) is None
    for bad in ("tv", "tv:", "tv:1:2:3", "tv:x", "l1:1e-3", "tv:-1", "tv:1e-3:-1"):
        opts, config = parse_cli(argv=["--config", plain, "--sense-prior", bad], extra_flags=add_sense_flags)
        with pytest.raises(ValueError, match="prior"):
            apply_sense_flags(config, opts)


# ---- header, binding, build --------------------------------------------------------------------------------------------
def test_header_binding_and_makefile():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_image_tv_grad\(const float\* img, int64_t H, int64_t W, float weight, float eps, "
                     r"int32_t accumulate,\s+float\* loss_out, float\* dimg, void\* stream\);", text, re.M)
    head = text[:text.index("#define INR_ABI_VERSION")]
    assert "inr_image_tv_grad" in head[head.index("v7 additions"):]
    assert hasattr(L.load(), "inr_image_tv_grad")  # the built library exports it
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7 and L.load().inr_abi_version() == 7
    assert len(L.SYMBOLS["inr_image_tv_grad"][1]) == 9
    assert "#define INR_IMAGE_TV_BLOCKS 255\n" in text and "#define INR_IMAGE_TV_PARTIALS 2\n" in text
    assert (L.IMAGE_TV_BLOCKS, L.IMAGE_TV_PARTIALS) == (255, 2)
    assert L.IMAGE_TV_PARTIALS + 2 * L.IMAGE_TV_BLOCKS <= L.LOSS_WORDS  # a trainer's loss buffer serves
    H, W = PC.LARGE  # the shared cases' large shape is the one the block constants ask for
    assert W % 2 == 1 and L.IMAGE_TV_BLOCKS * L.IMAGE_TV_THREADS < H * W <= 2 * L.IMAGE_TV_BLOCKS * L.IMAGE_TV_THREADS
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "inr_aux.h")) as f:
        aux = f.read()
    assert f"IMAGE_TV_THREADS = {L.IMAGE_TV_THREADS};" in aux and f"IMAGE_TV_BLOCKS = {L.IMAGE_TV_BLOCKS};" in aux
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert "inr_image_tv.hip" in make[make.index("SRCS :="):make.index("OBJS :=")]


def test_binding_refuses_host_tensors_and_bad_shapes():
    img = torch.zeros(30, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.image_tv(img, 6, 5, 1.0, 1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.image_tv(img, 6, 5, 1.0, 1e-3, dimg=torch.zeros(30, 2), accumulate=True)
    with pytest.raises(RuntimeError, match="shape"):
        P.image_tv(img, 5, 5, 1.0, 1e-3)
    with pytest.raises(RuntimeError, match="shape"):
        P.image_tv(img, 6, 5, 1.0, 1e-3, dimg=torch.zeros(30))
    with pytest.raises(RuntimeError, match="shape"):
        P.image_tv(img, 6, 5, 1.0, 1e-3, loss_out=torch.zeros(8))
    with pytest.raises(RuntimeError, match="dimg"):
        P.image_tv(img, 6, 5, 1.0, 1e-3, accumulate=True)
