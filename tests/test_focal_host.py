"""Focal frequency loss without a GPU (inr_mi355x/focal.py): the numpy statement of inr_focal_loss_grad
against the reference's FocalFrequencyLoss (tests/golden/focal.npz, made by tools/make_golden_focal.py: its loss and its
autograd gradient in float64 and fp32), the config keys, every refusal, and the entry in header, binding and Makefile."""
import json
import os
import re

import numpy as np
import pytest
import torch

import focal_cases as FC
from conftest import GOLDEN, ROOT

from inr_mi355x import _lib as L
from inr_mi355x import focal as Fo
from inr_mi355x.engine import LOSS_FOCAL_HOST, LossSpec
from inr_mi355x.focal import FocalSpec


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "focal_meta.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN, "focal.npz")), meta


def _case(z, c):
    out = z["gt"] if c["equal"] else z["out"]
    return FocalSpec(c["alpha"], c["log_matrix"], c["loss_weight"]), out, z["gt"], (z["mask"] if c["masked"] else None)


def test_fixture_holds_the_cases_of_the_issue(golden):
    z, meta = golden
    assert meta["B"] == 37 and z["out"].shape == (37, 2) and z["out"].dtype == np.float32
    assert set(meta["cases"]) == {"defaults", "alpha_0.5", "alpha_2", "no_log", "weight_0.3", "equal", "masked"}
    worst = int(np.argmax(((z["out"] - z["gt"]).astype(np.float64) ** 2).sum(1)))
    assert z["mask"][worst] == 0 and 0 < z["mask"].sum() < 37  # the masked case keeps the largest error OUT of n_max
    assert float(z["equal.loss64"]) == 0.0 and not z["equal.grad64"].any()  # 0 / 0 -> 0 in the reference, no NaN


def test_float64_statement_is_the_reference(golden):
    """loss and gradient at 1e-12 relative, every case; unsampled rows exactly 0"""
    z, meta = golden
    for name, c in meta["cases"].items():
        spec, out, gt, m = _case(z, c)
        loss, dout, n_max = Fo.focal_loss_numpy(spec, out, gt, c["count"], m)
        want_l, want_g = float(z[name + ".loss64"]), z[name + ".grad64"]
        assert abs(loss - want_l) <= 1e-12 * abs(want_l), (name, loss, want_l)
        assert np.all(np.abs(dout - want_g) <= 1e-12 * np.abs(want_g)), name
        if m is not None:
            assert not dout[m == 0].any() and not want_g[m == 0].any()
        assert (n_max == 0.0) == c["equal"]


def test_fp32_statement_against_the_reference_in_fp32(golden):
    """the fp32 mode lies within the derived bound (focal_cases.focal_ref) of float64, and within TWICE that bound of the
    reference's own fp32 run: both are fp32 evaluations of one expression with the same operations per element (the
    reference divides by N where the kernel multiplies by 1 / N), each within the bound of the float64 value -- the
    triangle inequality, nothing measured.  The F-class restatement of focal_cases gives the fp32 mode's bits."""
    z, meta = golden
    for name, c in meta["cases"].items():
        spec, out, gt, m = _case(z, c)
        loss, dout, n_max = Fo.focal_loss_numpy(spec, out, gt, c["count"], m, dtype=np.float32)
        assert dout.dtype == np.float32 and isinstance(loss, np.float32)
        ref = FC.focal_ref(out, gt, m, c["count"], c["alpha"], c["log_matrix"], c["loss_weight"])
        assert FC.C.ratio(dout, ref["dout"], ref["dout_bound"]) <= 1.0, name
        assert FC.C.ratio(loss, ref["loss"], ref["loss_bound"]) <= 1.0, name
        assert FC.C.ratio(n_max, ref["n_max"], ref["n_max_bound"]) <= 1.0, name
        assert FC.C.ratio(dout, z[name + ".grad32"], 2.0 * ref["dout_bound"]) <= 1.0, name
        assert FC.C.ratio(loss, z[name + ".loss32"], 2.0 * ref["loss_bound"]) <= 1.0, name
        # the bound is useful: far below the gradient it guards.  Relative to the LARGEST entry: a row of small error has
        # n = log(1 + m) from the rounded sum 1 + m, an absolute error of u whatever m is -- the formula's own conditioning
        assert np.all(ref["dout_bound"] <= 1e-5 * np.abs(ref["dout"]).max()), name
        # (the loss word's worst case is the chain of 265 additions: gamma(265) = 1.6e-5, plus the terms' own bounds)
        assert ref["loss_bound"] <= 2.0 * FC.C.gamma(FC.chain(37)) * abs(ref["loss"]) or ref["loss"] == 0.0
        terms, d32, nm32 = FC.focal_f32(out, gt, m, c["count"], c["alpha"], c["log_matrix"], c["loss_weight"])
        assert np.array_equal(d32, dout) and nm32 == n_max, name


def test_fold_is_the_kernels_partition():
    """_fold32 on terms that make the order visible: 255 blocks of pairs, lanes, tree, ordered partials"""
    for B in (1, 2, 257, 1000, 131073):
        t = np.abs(FC.rnd(B, 5, 1.0)) * np.float32(1e-3) + np.where(np.arange(B) % 97 == 0, np.float32(1.0), np.float32(0))
        t = t.astype(np.float32)
        live = np.ones(B, dtype=bool)
        got = Fo._fold32(t, live)
        pairs, f = (B + 1) // 2, np.float32
        per = -(-pairs // 255)
        tp = np.zeros(2 * pairs, dtype=f)
        tp[:B] = t
        total = f(0)
        for b in range(255):
            lanes = [f(0)] * 256
            for p in range(min(b * per, pairs), min((b + 1) * per, pairs)):
                j = (p - b * per) % 256
                lanes[j] = f(f(lanes[j] + tp[2 * p]) + tp[2 * p + 1])
            s = 128
            while s:
                lanes[:s] = [f(lanes[i] + lanes[i + s]) for i in range(s)]
                s //= 2
            total = f(total + lanes[0])
        assert got == total and got.dtype == np.float32, B
        assert abs(float(got) - float(t.astype(np.float64).sum())) <= FC.C.gamma(FC.chain(B)) * float(t.sum())


def test_spec_parsing():
    assert FocalSpec.from_opts(None) == FocalSpec(1.0, True, 1.0) == FocalSpec.from_opts({})
    assert FocalSpec.from_opts({"hdr_eps": 1e-3}) == FocalSpec()  # the other losses' keys may stay in loss_opts
    s = FocalSpec.from_opts({"ffl_alpha": 0.5, "ffl_log_matrix": False, "ffl_weight": 0.3})
    assert s == FocalSpec(0.5, False, 0.3) and s.summary() == {"alpha": 0.5, "log_matrix": False, "loss_weight": 0.3}
    for bad in ({"ffl_alpha": 0.0}, {"ffl_alpha": -1.0}, {"ffl_alpha": float("nan")}, {"ffl_alpha": float("inf")},
                {"ffl_weight": float("inf")}, {"ffl_log_matrix": "yes"}, {"ffl_batch_matrix": True}, {"ffl_alhpa": 1.0}):
        with pytest.raises(ValueError, match="ffl_"):
            FocalSpec.from_opts(bad)


def test_loss_spec_from_config():
    spec = LossSpec.from_config({"loss": "FFL", "loss_opts": {"ffl_alpha": 2.0}})
    assert spec.kind == LOSS_FOCAL_HOST == -1 and spec.focal == FocalSpec(2.0, True, 1.0)
    assert spec.kind not in (L.LOSS_L2_HALF, L.LOSS_L1_HALF, L.LOSS_TANH, L.LOSS_LOGSPACE, L.LOSS_HDR, L.LOSS_MSLE_HALF,
                             L.LOSS_CENTER)  # a host-side marker: the C enum has no new value
    assert LossSpec.from_config({"loss": "FFL"}).focal == FocalSpec()
    assert LossSpec.from_config({"loss": "L2"}).focal is None
    with pytest.raises(ValueError, match="ffl_gamma"):
        LossSpec.from_config({"loss": "FFL", "loss_opts": {"ffl_gamma": 1.0}})
    with pytest.raises(NotImplementedError, match="FFL"):  # the list of what IS supported names it
        LossSpec.from_config({"loss": "T"})


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="FFL", lr=1e-3, batch_size=100, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


REFUSALS = [
    (dict(), dict(rank=0, world=2), "more than one rank"),
    (dict(per_coil=True), {}, "per_coil"),
    (dict(use_tv=True), {}, "use_tv"),
    (dict(model="Fourier"), {}, "filter networks"),
    (dict(model="Gabor"), {}, "filter networks"),
    (dict(model="KGabor"), {}, "filter networks"),
    (dict(precision="bf16"), {}, "precision"),
]


@pytest.mark.parametrize("cfg_kw, ctor_kw, match", REFUSALS, ids=[r[2].replace(" ", "_") + str(i) for i, r in enumerate(REFUSALS)])
def test_trainer_refuses_before_any_device_call(cfg_kw, ctor_kw, match):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 8, 8)
    with pytest.raises(NotImplementedError, match=match):
        INRTrainer(_cfg(**cfg_kw), image, coords, shape, "cuda:0", **ctor_kw)


def test_other_drivers_refuse_before_any_device_call():
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    from inr_mi355x.train_scaling import ScaledFitTrainer
    image, coords, shape = make_kspace(2, 8, 8)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    with pytest.raises(NotImplementedError, match="FFL"):
        ScaledFitTrainer(_cfg(scaler=dict(network_width=32, network_depth=3)), image, coords, shape, "cuda:0")
    with pytest.raises(NotImplementedError, match="FFL"):
        MultiscaleTrainer(_cfg(model="MultiscaleKFourier"), image, coords, dist, None, shape, "cuda:0")
    with pytest.raises(NotImplementedError, match="FFL"):
        RingEnsembleTrainer(_cfg(), image, coords, shape, "cuda:0")


def test_hp_search_accepts_the_name():
    from inr_mi355x.hp_search import check_search
    check_search(_cfg(), {"method": "grid", "search_space": {"loss": {"values": ["L2", "FFL"]}}})


def test_header_binding_and_makefile():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^typedef struct \{ float alpha; int32_t log_matrix; float loss_weight; float inv_count; \} "
                     r"inr_focal_desc;", text, re.M)
    assert re.search(r"^int inr_focal_loss_grad\(const inr_focal_desc\* d, const float\* out, const float\* gt, "
                     r"const uint8_t\* mask,\s+int64_t B, float\* loss_out, float\* dout, void\* stream\);", text, re.M)
    head = text[:text.index("#define INR_ABI_VERSION")]
    assert "inr_focal_loss_grad" in head[head.index("v7 additions"):]  # listed under the v7 additions; the version stays
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7 and L.load().inr_abi_version() == 7
    decl = text.index("int inr_focal_loss_grad(")
    assert "(v7 addition)" in text[text.rindex("/*", 0, decl):decl]
    assert hasattr(L.load(), "inr_focal_loss_grad")  # the built library exports it
    assert len(L.SYMBOLS["inr_focal_loss_grad"][1]) == 8
    import ctypes
    assert ctypes.sizeof(L.FocalDesc) == 16 and [f[0] for f in L.FocalDesc._fields_] == ["alpha", "log_matrix", "loss_weight",
                                                                                         "inv_count"]
    words = {k: int(re.search(rf"^#define INR_FOCAL_{k} (\d+)", text, re.M).group(1)) for k in
             ("BLOCKS", "PARTIALS", "MAXIMA", "NMAX")}
    assert (words["BLOCKS"], words["PARTIALS"], words["MAXIMA"], words["NMAX"]) == \
        (L.FOCAL_BLOCKS, L.FOCAL_PARTIALS, L.FOCAL_MAXIMA, L.FOCAL_NMAX) and FC.BLOCKS == L.FOCAL_BLOCKS
    assert words["PARTIALS"] + words["BLOCKS"] <= words["MAXIMA"] and words["MAXIMA"] + words["BLOCKS"] <= words["NMAX"] \
        and words["NMAX"] < L.LOSS_WORDS  # the words do not overlap and fit the buffer
    assert "#define INR_LOSS_WORDS 512\n" in text  # nothing existing moved
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        assert "inr_loss_focal.hip" in f.read()


def test_bindings_refuse_host_tensors_and_bad_shapes():
    out, gt = torch.zeros(4, 2), torch.zeros(4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fo.focal_loss_grad(FocalSpec(), out, gt, 4)
    with pytest.raises(RuntimeError, match="shape"):
        Fo.focal_loss_grad(FocalSpec(), torch.zeros(4, 3), gt, 4)
    with pytest.raises(RuntimeError, match="shape"):
        Fo.focal_loss_grad(FocalSpec(), out, torch.zeros(3, 2), 4)
    with pytest.raises(RuntimeError, match="shape"):
        Fo.focal_loss_grad(FocalSpec(), out, gt, 4, mask=torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="shape"):
        Fo.focal_loss_grad(FocalSpec(), torch.zeros(8), gt, 4)
    with pytest.raises(RuntimeError, match="count"):
        Fo.focal_loss_grad(FocalSpec(), out, gt, 0)


def test_shipped_config_and_command_line(tmp_path):
    from inr_mi355x.cli import get_config, parse_cli
    path = os.path.join(ROOT, "configs", "config_siren_kspace_ffl.yaml")
    cfg = get_config(path)
    assert cfg["loss"] == "FFL" and cfg["loss_opts"] == {"ffl_alpha": 1.0, "ffl_log_matrix": True, "ffl_weight": 1.0}
    assert LossSpec.from_config(cfg).focal == FocalSpec()
    base = get_config(os.path.join(ROOT, "configs", "config_siren_kspace.yaml"))
    assert {k: v for k, v in cfg.items() if k not in ("loss", "loss_opts")} == \
        {k: v for k, v in base.items() if k not in ("loss", "loss_opts")}  # BASELINE config 2 but for the loss
    opts, config = parse_cli(argv=["--config", path, "--synthetic", "2,16,24", "--val", "--shuffle", "--band-report", "10",
                                   "--output_path", str(tmp_path)])
    assert config["loss"] == "FFL" and opts.val
