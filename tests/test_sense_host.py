"""SENSE-model fits, the part that needs no GPU: the shift permutation against torch.fft.ifftshift, the
fp32 numpy text of the two kernels against the float64 chain, the float64 chain against torch float64 autograd of
loss(fft2c(scale * S * I)) for every loss kind inr_loss_grad takes, the trainer's refusals, the ``sense`` key, the
checkpoint keys, and the header / binding / Makefile entries."""
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as C
import oracle as O
import sense_cases as SC
from aux_bits_cases import rnd
from conftest import ROOT

from inr_mi355x import _lib as L
from inr_mi355x import sense as S
from inr_mi355x.engine import LossSpec

OPTS = dict(hdr_eps=C.EPS, hdr_ff_sigma=2.0, hdr_ff_factor=C.FACTOR, min_sample=4)
f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).copy())
TOL = 1e-5  # the project's plain criterion: relative L2 per array


def _spec(kind):
    return LossSpec(C.KINDS[kind], C.EPS, 2.0, C.FACTOR, 3000)


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.abs(got).max(initial=0.0))


def _oracle(kind, y, t, kc):
    """scale * loss_fn of the reference's loops (train.py:176-182), as tests/test_gain_host.py calls the oracle"""
    if kind == "l2":
        return O.loss_l2_half(y, t)
    if kind == "l1":
        return O.loss_l1_half(y, t)
    if kind == "tanh":
        return O.loss_tanh(y, t)[0]
    if kind == "logspace":
        return O.loss_logspace(y, t, OPTS)
    if kind == "msle":
        return 0.5 * O.loss_msle(y, t)
    if kind == "hdr":
        return O.loss_hdr(y, t, kc, OPTS)[0]
    return O.loss_center(y, t, kc, OPTS)[0]  # kcoords outside both bands: the pointwise part alone


# ---- the shift ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", SC.PARITIES)
@pytest.mark.parametrize("W", SC.PARITIES)
def test_shift_index_is_ifftshift(H, W):
    plane = torch.arange(H * W).reshape(H, W)
    want = torch.fft.ifftshift(plane, dim=(0, 1)).reshape(-1).numpy()
    perm = S.shift_index(H, W)
    assert perm.dtype == np.int64 and np.array_equal(perm, want)
    place = S.place_index(H, W)
    assert np.array_equal(perm[place], np.arange(H * W)) and np.array_equal(place[perm], np.arange(H * W))
    # ... and the kernels' text stores pixel p at place[p]: shift = 1 is ifftshift of shift = 0
    img, sens, _ = SC.inputs(2, H, W)
    x0 = S.sense_apply_numpy(img, sens, 2, H, W, SC.SCALE, 0)
    x1 = S.sense_apply_numpy(img, sens, 2, H, W, SC.SCALE, 1)
    want1 = torch.fft.ifftshift(torch.from_numpy(x0), dim=(1, 2)).numpy()
    assert np.array_equal(x1.view(np.int32), want1.view(np.int32))


# ---- the fp32 text against the float64 chain, the chain against autograd -----------------------------------------------
@pytest.mark.parametrize("shape", SC.HOST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_text_against_the_float64_chain(shape):
    """x of sense_apply_numpy against the chain's X, (dimg, dsens) of sense_grad_numpy on the chain's gX against the
    chain's.  Bound, reasoned: every output is at most four fp32 operations behind its inputs (dimg: G + 3), each within
    2^-24 relative of a partial result no larger than the sum of the magnitudes that enter, and gX is rounded to fp32
    once more: (G + 4) * 2^-23 relative L2 covers it.  shift = 1 gives the bits of shift = 0, permuted."""
    G, H, W = shape
    img, sens, _ = SC.inputs(G, H, W)
    gt, m, count = SC.targets("l2", G, H, W, "random")
    _, dimg, dsens, X, gX = S.sense_chain_numpy(img, sens, gt, m, _spec("l2"), count, G, H, W, SC.SCALE, parts=True)
    bound = (G + 4) * 2.0 ** -23
    x0 = S.sense_apply_numpy(img, sens, G, H, W, SC.SCALE, 0)
    assert x0.dtype == np.float32 and x0.shape == (G, H, W, 2) and rel_l2(x0, X) <= bound
    g32 = gX.astype(np.float32)
    di, ds = S.sense_grad_numpy(img, sens, g32, G, H, W, SC.SCALE, 0)
    assert di.dtype == ds.dtype == np.float32 and di.shape == (H * W, 2) and ds.shape == (G * H * W, 2)
    assert np.linalg.norm(dimg) > 0 and rel_l2(di, dimg) <= bound and rel_l2(ds, dsens) <= bound
    perm = S.shift_index(H, W)
    x1 = S.sense_apply_numpy(img, sens, G, H, W, SC.SCALE, 1)
    assert np.array_equal(x1.reshape(G, H * W, 2), x0.reshape(G, H * W, 2)[:, perm])
    di1, ds1 = S.sense_grad_numpy(img, sens, g32.reshape(G, H * W, 2)[:, perm], G, H, W, SC.SCALE, 1)
    assert np.array_equal(di1.view(np.int32), di.view(np.int32)) and np.array_equal(ds1.view(np.int32), ds.view(np.int32))


@pytest.mark.parametrize("kind", list(C.KINDS))
def test_chain_is_autograd_in_float64(kind):
    """loss, dimg and dsens of sense_chain_numpy against torch float64 autograd of loss(fft2c(scale * S * I)) over the
    sampled rows: 1e-5 relative on the loss, 1e-5 relative L2 per array (the plain criterion); an all-zero mask gives
    loss 0 and no gradient."""
    for G, H, W in SC.HOST_SHAPES:
        img, sens, _ = SC.inputs(G, H, W)
        n = G * H * W
        for tag in SC.MASKS:
            gt, m, count = SC.targets(kind, G, H, W, tag)
            keep = np.ones(n, dtype=bool) if m is None else m != 0
            rows = int(keep.sum())
            kc = np.zeros((rows, 3))
            kc[:, 1], kc[:, 2] = (2.0, 0.0) if kind == "center" else (rnd(rows, 40, 1.0), rnd(rows, 41, 1.0))
            kc = f64(kc)
            A = float(torch.mean((1.0 - torch.exp(-(kc[:, 1] ** 2 + kc[:, 2] ** 2) / (2 * 2.0 ** 2))) ** 2)) if rows else 0.0
            got = S.sense_chain_numpy(img, sens, gt, m, _spec(kind), count, G, H, W, SC.SCALE, hdr_A=A)
            if rows == 0:
                assert got[0] == 0.0 and not got[1].any() and not got[2].any()
                continue
            it, st = f64(img).requires_grad_(True), f64(sens).requires_grad_(True)
            I = torch.view_as_complex(it.reshape(H, W, 2))
            Sm = torch.view_as_complex(st.reshape(G, H, W, 2))
            K = O.fft2c(torch.view_as_real(SC.SCALE * Sm * I[None])).reshape(n, 2)
            sel = torch.from_numpy(keep)
            loss = _oracle(kind, K[sel], f64(gt)[sel], kc)
            gi, gs = torch.autograd.grad(loss, (it, st))
            want = float(loss.detach())
            errs = dict(loss=abs(got[0] - want) / abs(want), dimg=rel_l2(got[1], gi.numpy()), dsens=rel_l2(got[2], gs.numpy()))
            assert np.linalg.norm(gi.numpy()) > 0 and np.linalg.norm(gs.numpy()) > 0
            for k, v in errs.items():
                assert v <= TOL, (kind, (G, H, W), tag, k, v)
            assert got[1].shape == (H * W, 2) and got[2].shape == (n, 2)


# ---- the trainer's refusals and keys -----------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=100, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               sense=dict(net=dict(network_width=32, network_depth=3)))
    cfg.update(kw)
    return cfg


REFUSALS = [
    (dict(transform=True), {}, "transform"),
    (dict(trajectory="radial-8"), {}, "trajectory"),
    (dict(ring_normalization="max"), {}, "ring_normalization"),
    (dict(row_sampling="ring-inverse"), {}, "row_sampling"),
    (dict(per_coil=True), {}, "per_coil"),
    (dict(use_tv=True), {}, "use_tv"),
    (dict(virtual_coils=2), {}, "virtual_coils"),
    (dict(loss="LSL"), {}, "LSL"),
    (dict(loss="FFL"), {}, "FFL"),
    (dict(regularization=dict(type="L2", strenght=1e-4)), {}, "regularization"),
    (dict(precision="bf16"), {}, "precision"),
    (dict(model="Fourier"), {}, "filter networks"),
    (dict(model="Gabor"), {}, "filter networks"),
    (dict(model="KGabor"), {}, "filter networks"),
    ({}, dict(graph_steps=True), "graph_steps"),
    ({}, dict(rank=0, world=2), "one rank"),
]


@pytest.mark.parametrize("cfg_kw, ctor_kw, match", REFUSALS, ids=[r[2] + str(i) for i, r in enumerate(REFUSALS)])
def test_trainer_refuses_before_any_device_call(cfg_kw, ctor_kw, match):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    image, coords, shape = make_kspace(2, 8, 8)
    with pytest.raises(NotImplementedError, match=match):
        SenseFitTrainer(_cfg(**cfg_kw), image, coords, shape, "cuda:0", **ctor_kw)


def test_sense_key():
    from inr_mi355x.train_sense import MAX_STASH_BYTES, coil_groups, sense_settings
    enc = dict(embedding="gauss", scale=4, embedding_size=256, coordinates_size=3)
    d = sense_settings({"encoder": enc}, n_coils=15)
    assert MAX_STASH_BYTES == 8 * 10 ** 9
    assert d == dict(coils_per_step=15, scale=None, net=dict(network_width=64, network_depth=4),
                     encoder=dict(scale=1.0, embedding_size=256), max_stash_bytes=MAX_STASH_BYTES)
    d = sense_settings({"encoder": enc, "sense": {"coils_per_step": 4, "scale": 0.01, "net": {"network_width": 32},
                                                  "encoder": {"scale": 2, "embedding_size": 8},
                                                  "max_stash_bytes": 1000}}, n_coils=15)
    assert d == dict(coils_per_step=4, scale=0.01, net=dict(network_width=32, network_depth=4),
                     encoder=dict(scale=2.0, embedding_size=8), max_stash_bytes=1000)
    assert sense_settings({"encoder": enc, "sense": {"coils_per_step": 40}}, n_coils=15)["coils_per_step"] == 15
    assert sense_settings({"encoder": enc})["coils_per_step"] is None
    for bad in ({"coils": 3}, {"net": {"network_input_size": 3}}, {"encoder": {"embedding": "LogF"}}, {"coils_per_step": 0},
                {"net": {"network_depth": 1}}, {"scale": float("inf")}, {"scale": 0.0}, {"max_stash_bytes": 0}):
        with pytest.raises(ValueError, match="sense"):
            sense_settings({"encoder": enc, "sense": bad}, n_coils=15)
    assert coil_groups(3, 3) == [(0, 3)] and coil_groups(3, 2) == [(0, 2), (2, 3)] and coil_groups(15, 4)[-1] == (12, 15)


def test_checkpoint_key_split_and_join():
    from inr_mi355x.train_sense import has_sense_keys, join_state, split_state
    img = {"model.0.linear.weight": torch.ones(2, 3), "model.0.linear.bias": torch.zeros(2)}
    sen = {"model.0.weight": torch.full((2, 3), 2.0), "model.0.bias": torch.zeros(2)}
    net = join_state(img, sen)
    assert list(net) == ["image.model.0.linear.weight", "image.model.0.linear.bias", "sens.model.0.weight", "sens.model.0.bias"]
    assert has_sense_keys(net) and not has_sense_keys(img) and not has_sense_keys({"backbone.x": 1, "scaler.y": 2})
    assert net["image.model.0.linear.weight"].data_ptr() != img["model.0.linear.weight"].data_ptr()  # clones
    a, b = split_state(net)
    assert list(a) == list(img) and list(b) == list(sen)
    assert all(torch.equal(a[k], img[k]) for k in img) and all(torch.equal(b[k], sen[k]) for k in sen)
    with pytest.raises(ValueError, match="outside"):
        split_state(dict(net, **{"scaler.model.0.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="both"):
        split_state({k: v for k, v in net.items() if k.startswith("image.")})


def test_header_binding_and_makefile():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_sense_apply\(const float\* img, const float\* sens, int32_t G, int64_t H, int64_t W, "
                     r"float scale,\s+int32_t shift,\s+float\* x, void\* stream\);", text, re.M)
    assert re.search(r"^int inr_sense_grad\(const float\* img, const float\* sens, const float\* gx, int32_t G, int64_t H, "
                     r"int64_t W, float scale,\s+int32_t shift, float\* dimg, float\* dsens, void\* stream\);", text, re.M)
    head = text[:text.index("#define INR_ABI_VERSION")]
    for name in ("inr_sense_apply", "inr_sense_grad"):
        assert name in head[head.index("v7 additions"):]  # listed under the v7 additions; the version stays
        assert hasattr(L.load(), name)  # the built library exports it
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7 and L.load().inr_abi_version() == 7
    decl = text.index("int inr_sense_apply(")
    assert "(v7 additions)" in text[text.rindex("/*", 0, decl):decl]
    assert len(L.SYMBOLS["inr_sense_apply"][1]) == 9 and len(L.SYMBOLS["inr_sense_grad"][1]) == 11
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        assert "inr_sense.hip" in f.read()


def test_bindings_refuse_host_tensors_and_bad_shapes():
    img, sens, gx = torch.zeros(6, 2), torch.zeros(12, 2), torch.zeros(2, 2, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.sense_apply(img, sens, 2, 2, 3, 1.0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.sense_grad(img, sens, gx, 2, 2, 3, 1.0, 1)
    with pytest.raises(RuntimeError, match="shape"):
        S.sense_apply(img, torch.zeros(6, 2), 2, 2, 3, 1.0, 1)
    with pytest.raises(RuntimeError, match="shape"):
        S.sense_grad(img, sens, torch.zeros(2, 3, 2, 2), 2, 2, 3, 1.0, 1)


def test_command_line_and_config():
    """the module CLI takes train_scaling's flags, and configs/config_siren_sense.yaml parses to the defaults it states"""
    from inr_mi355x.cli import parse_cli
    from inr_mi355x.train_sense import check_sense_config, sense_settings
    path = os.path.join(ROOT, "configs", "config_siren_sense.yaml")
    opts, config = parse_cli(argv=["--config", path, "--synthetic", "15,640,368", "--max_steps", "3", "--val",
                                   "--save-images", "--shuffle", "--shuffle-seed", "5", "--band-report", "10",
                                   "--output_path", "out"])
    assert config["undersampling"] == "grid-3*2" and config["shuffle"] and config["shuffle_seed"] == 5
    check_sense_config(config)
    d = sense_settings(config, n_coils=15)
    assert d.pop("coils_per_step") == 5  # three groups: all 15 coils at once are beyond the stash budget at the brain shape
    defaults = sense_settings({k: v for k, v in config.items() if k != "sense"}, n_coils=15)
    assert defaults.pop("coils_per_step") == 15 and d == defaults  # the rest of the block spells the defaults
