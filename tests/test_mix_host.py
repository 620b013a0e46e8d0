"""Mixture of heads, host side (no GPU): the float64 statement of inr_mi355x/mix.py against
torch.autograd of the batch loss written out with the oracle's loss functions, the clamp's and the rings' edge rules, the
config refusals, the checkpoint's key names, the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as C
import mix_cases as MC
import oracle as O
from conftest import ROOT

from inr_mi355x import _lib as L
from inr_mi355x import mix as M
from inr_mi355x.engine import LossSpec

OPTS = dict(hdr_eps=C.EPS, hdr_ff_sigma=2.0, hdr_ff_factor=C.FACTOR, min_sample=4)
f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def _spec(kind):
    return LossSpec(C.KINDS[kind], C.EPS, 2.0, C.FACTOR, 3000)


def _oracle(kind, y, t, kc):
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
    return O.loss_center(y, t, kc, OPTS)[0]


def _kc(kind, n):
    """k-space coordinates of n rows at ONE radius: the losses' scalar A is then the same for every subset of rows, as
    the statement's single hdr_A (center: outside both bands, the pointwise part alone)"""
    kc = np.zeros((n, 3))
    kc[:, 1] = 2.0 if kind == "center" else 1.3
    kc = f64(kc)
    A = float(torch.mean((1.0 - torch.exp(-(kc[:, 1] ** 2 + kc[:, 2] ** 2) / (2 * 2.0 ** 2))) ** 2))
    return kc, A


def _close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert got.shape == want.shape and np.all(err <= rel * np.abs(want)), \
        (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))


def _autograd(kind, ys, w, gt, dist, mask, radii, detach, clamp):
    """(total, terms, res, dys, dw) of the issue's statement by torch.autograd in float64"""
    K, B = len(ys), len(gt)
    yt = [f64(y).requires_grad_(True) for y in ys]
    wt = f64(w).requires_grad_(True)
    live = np.ones(B, dtype=bool) if mask is None else mask != 0
    pre = None
    for k in range(K):
        term = wt[:, k:k + 1] * (yt[k].detach() if detach else yt[k])
        pre = term if pre is None else pre + term
    res = torch.clamp(pre, -1.0, 1.0) if clamp else pre
    terms = []
    sel = torch.from_numpy(live)
    kc, _ = _kc(kind, int(live.sum()))
    terms.append(_oracle(kind, res[sel], f64(gt)[sel], kc) if live.any() else res.sum() * 0.0)
    rings = M.ring_membership(dist, radii)
    for k in range(K):
        s = live & rings[k]
        kc, _ = _kc(kind, int(s.sum()))
        st = torch.from_numpy(s)
        terms.append(_oracle(kind, yt[k][st], f64(gt)[st], kc) if s.any() else yt[k].sum() * 0.0)
    total = sum(terms)
    grads = torch.autograd.grad(total, yt + [wt], allow_unused=True)
    z = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()
    return (float(total.detach()), [float(t.detach()) for t in terms], res.detach().numpy(),
            [z(g, ys[0]) for g in grads[:K]], z(grads[K], w))


CASES = [(0.3, True), (0.3, False), (1.0, True)]  # |res| and |y_k| stay where 1 - tanh^2 keeps its digits in float64


@pytest.mark.parametrize("kind", list(C.KINDS))
def test_numpy_statement_is_autograd_in_float64(kind):
    """total, each term, res, every dy_k and dw of mix_loss_grad_numpy against torch.autograd in float64, 1e-12 relative
    per element, for both detach values and both clamp values; unsampled rows are exactly 0"""
    _, A = _kc(kind, 1)
    for B in (1, 63, 257):
        for K in (2, 3):
            for amp, clamp in CASES:
                ys, w, gt, dist, radii = MC.rows(kind, B, K, amp)
                for tag in ("none", "random"):
                    m = MC.mask_of(tag, B)
                    for detach in (True, False):
                        want = _autograd(kind, ys, w, gt, dist, m, radii, detach, clamp)
                        got = M.mix_loss_grad_numpy(_spec(kind), ys, w, gt, dist, m, radii, detach=detach, clamp=clamp,
                                                    hdr_A=A)
                        what = (kind, B, K, amp, clamp, tag, detach)
                        _close(got[0], want[0], what + ("total",))
                        _close(got[1], want[1], what + ("terms",))
                        _close(got[3], want[2], what + ("res",))
                        for k in range(K):
                            _close(got[4][k], want[3][k], what + ("dy", k))
                        _close(got[5], want[4], what + ("dw",))
                        if m is not None:
                            assert not got[5][m == 0].any() and not any(d[m == 0].any() for d in got[4])


def test_clamp_passes_the_gradient_at_exactly_one():
    """w = (0.5, 0.5), y = +-1: pre is exactly +-1, and the gradient passes as torch.clamp's does; just beyond it does not"""
    ys = [np.array([[1.0, -1.0], [1.0, 1.0]], dtype=np.float32)] * 2
    w = np.array([[0.5, 0.5], [0.5, 0.5 + 2.0 ** -20]], dtype=np.float32)
    gt = np.array([[0.25, 0.5], [0.25, 0.5]], dtype=np.float32)
    dist, radii = np.array([0.1, 0.1], dtype=np.float32), [0.0, 0.5, 1.0]
    got = M.mix_loss_grad_numpy(_spec("l2"), ys, w, gt, dist, None, radii, detach=True, clamp=True)
    want = _autograd("l2", ys, w, gt, dist, None, radii, True, True)
    assert got[2][0].tolist() == [1.0, -1.0] and got[3][0].tolist() == [1.0, -1.0]
    assert got[5][0, 0] != 0.0 and got[5][0, 1] != 0.0           # row 0: pre == +-1 exactly, the gradient passes
    assert (got[2][1] > 1.0).all() and not got[5][1].any()       # row 1: both components above 1, nothing passes
    _close(got[5], want[4], "dw")
    pre32, res32 = M.mix_numpy_f32(ys, w, True)
    assert pre32[0].tolist() == [1.0, -1.0] and res32[1].tolist() == [1.0, 1.0] and pre32.dtype == np.float32


def test_edge_rows_count_in_both_rings_and_an_empty_ring_adds_nothing():
    radii = [0.0, 0.5, 1.0, 1.5]
    dist = np.array([0.5, 0.25, 0.25, 1.5, 2.0], dtype=np.float32)  # row 0 on the edge of rings 0 / 1; row 4 in no ring
    mask = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    assert M.ring_counts(dist, None, radii) == [5, 3, 1, 1]
    assert M.ring_counts(dist, mask, radii) == [4, 2, 1, 1]
    assert M.ring_counts(dist, mask, radii, 1, 3) == [1, 1, 0, 0]
    assert M.ring_counts(torch.from_numpy(dist), torch.from_numpy(mask), radii) == [4, 2, 1, 1]
    assert M.inv_counts([4, 2, 0, 1]) == [0.25, 0.5, 0.0, 1.0]
    ys = [MC.rnd(10, 7 + k, 0.3).reshape(5, 2) for k in range(3)]
    w, gt = MC.rnd(15, 11, 1.0).reshape(5, 3), MC.rnd(10, 12, 0.3).reshape(5, 2)
    total, terms, _, _, dys, dw = M.mix_loss_grad_numpy(_spec("l2"), ys, w, gt, dist, None, radii)
    assert dys[0][0].any() and dys[1][0].any() and not dys[2][0].any()      # the edge row trains experts 0 and 1
    assert not any(d[4].any() for d in dys) and dw[4].any()                  # outside every ring: the gate alone
    # ring 1 emptied: its term is exactly 0, its expert gets no gradient, the other terms keep their bits
    dist2 = dist.copy()
    dist2[[0]] = 0.25
    total2, terms2, _, _, dys2, _ = M.mix_loss_grad_numpy(_spec("l2"), ys, w, gt, dist2, None, radii)
    assert M.ring_counts(dist2, None, radii) == [5, 3, 0, 1]
    assert terms2[2] == 0.0 and not dys2[1].any() and terms2[0] == terms[0] and terms2[3] == terms[3]
    assert total2 == sum(terms2)


def test_chosen_seeds_stay_under_the_near_clamp_cap():
    """tests/test_gpu_mix.py leaves rows whose float64 |pre_c| lies within 1e-6 of 1 out of its dy / dw comparison and caps
    them at 1 % of the rows: with the inputs of mix_cases.py there are none at all (and at the large size the clamp does
    act in the 1.0 set and is idle in neither)"""
    for kind in ("l2", "msle"):
        for B in MC.SIZES:
            for K in MC.HEADS:
                for amp in MC.AMPS:
                    ys, w, gt, dist, radii = MC.rows(kind, B, K, amp)
                    pre = M.mix_loss_grad_numpy(_spec(kind), ys, w, gt, dist, None, radii)[2]
                    near = MC.near_clamp(pre)
                    assert near.sum() <= MC.NEAR_CAP * B, (kind, B, K, amp, int(near.sum()))
                    if B == 16385 and amp == 1.0:
                        assert (np.abs(pre) > 1.0).mean() > 0.05
                    if B == 63:
                        assert M.ring_counts(dist, None, radii)[2] == 0
                    if B >= 255:
                        r32 = np.asarray(radii, dtype=np.float32)
                        assert (dist == r32[1]).any() and min(M.ring_counts(dist, None, radii)) > 0


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=100, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               partition=dict(no_steps=20, no_models=3), mixture=dict(gate=dict(network_width=16, network_depth=3)))
    cfg.update(kw)
    return cfg


REFUSALS = [
    (dict(model="Fourier"), {}, "filter networks"),
    (dict(model="Gabor"), {}, "filter networks"),
    (dict(model="KGabor"), {}, "filter networks"),
    (dict(precision="bf16"), {}, "precision"),
    (dict(per_coil=True), {}, "per_coil"),
    (dict(use_tv=True), {}, "use_tv"),
    (dict(loss="LSL"), {}, "LSL"),
    (dict(loss="FFL"), {}, "FFL"),
    (dict(regularization=dict(type="L2", strenght=1e-4)), {}, "regularization"),
    (dict(trajectory="radial-8"), {}, "trajectory"),
    (dict(ring_normalization="max"), {}, "ring_normalization"),
    (dict(row_sampling="ring-inverse"), {}, "row_sampling"),
    ({}, dict(graph_steps=True), "graph_steps"),
    ({}, dict(rank=0, world=2), "one rank"),
    (dict(partition=dict(no_steps=20, no_models=1)), {}, "1 heads"),
    (dict(partition=dict(no_steps=20, no_models=9)), {}, "9 heads"),
    ({}, dict(radii=[0.0, 1.0]), "1 heads"),
]


@pytest.mark.parametrize("cfg_kw, ctor_kw, match", REFUSALS, ids=[r[2] + str(i) for i, r in enumerate(REFUSALS)])
def test_trainer_refuses_before_any_device_call(cfg_kw, ctor_kw, match):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_multihead import MixtureFitTrainer
    image, coords, shape = make_kspace(2, 8, 8)
    with pytest.raises(NotImplementedError, match=match):
        MixtureFitTrainer(_cfg(**cfg_kw), image, coords, shape, "cuda:0", **ctor_kw)


def test_mixture_settings():
    from inr_mi355x.train_multihead import GATE_NET, gate_net, mixture_settings
    s = mixture_settings({})
    assert s == dict(detach=True, clamp=True, gate=dict(network_width=128, network_depth=5))
    assert gate_net(s, 4) == dict(network_input_size=2, network_output_size=4, network_depth=5, network_width=128)
    assert GATE_NET == dict(network_input_size=2, network_depth=5, network_width=128)
    s = mixture_settings(dict(mixture=dict(detach=False, clamp=False, gate=dict(network_width=16))))
    assert s == dict(detach=False, clamp=False, gate=dict(network_width=16, network_depth=5))
    for bad in (dict(heads=3), dict(gate=dict(width=3)), dict(gate=dict(network_depth=1))):
        with pytest.raises(ValueError):
            mixture_settings(dict(mixture=bad))


def test_checkpoint_keys_round_trip():
    import inr_mi355x as P
    from inr_mi355x.train_multihead import gate_net, has_head_keys, merge_state, mixture_settings, split_state, wrong_checkpoint
    net = _cfg()["net"]
    torch.manual_seed(0)
    experts = [P.SIREN(net) for _ in range(3)]
    gate = P.FFN(gate_net(mixture_settings(_cfg()), 3))
    merged = merge_state([m.state_dict() for m in experts], gate.state_dict())
    # the names torch gives a wrapper that holds its heads in a ModuleList
    wrapper = torch.nn.Module()
    wrapper.heads = torch.nn.ModuleList(experts)
    wrapper.weighted_avg = gate
    assert list(merged) == list(wrapper.state_dict())
    assert [k for k in merged if k.startswith("weighted_avg.")][:2] == ["weighted_avg.model.0.weight",
                                                                        "weighted_avg.model.0.bias"]
    assert has_head_keys(merged) and not has_head_keys(experts[0].state_dict())
    heads, g = split_state(merged)
    assert len(heads) == 3 and list(g) == list(gate.state_dict())
    for sd, m in zip(heads, experts):
        assert list(sd) == list(m.state_dict()) and all(torch.equal(sd[k], v) for k, v in m.state_dict().items())
    again = merge_state(heads, g)
    assert list(again) == list(merged) and all(torch.equal(again[k], merged[k]) for k in merged)
    assert merged["heads.0.model.0.linear.weight"].data_ptr() != experts[0].state_dict()["model.0.linear.weight"].data_ptr()
    with pytest.raises(ValueError, match="outside"):
        split_state(dict(merged, other=torch.zeros(1)))
    with pytest.raises(ValueError, match="heads"):
        split_state({k: v for k, v in merged.items() if not k.startswith("heads.1.")})
    assert "train_scaling" in wrong_checkpoint({"scaler.model.0.weight": 0, "backbone.x": 0})
    assert "inr_mi355x.train)" in wrong_checkpoint(experts[0].state_dict())


def test_header_binding_and_makefile():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_mix_loss_grad\(const inr_loss_desc\* loss, const inr_mix_desc\* mix, const float\* w,", text,
                     re.M)
    assert re.search(r"^int inr_mix_apply\(const inr_mix_desc\* mix, const float\* w, int64_t B, float\* res, "
                     r"void\* stream\);", text, re.M)
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7 and L.load().inr_abi_version() == 7
    decl = text.index("int inr_mix_loss_grad(")
    assert "(v7 additions)" in text[text.rindex("/*", 0, decl):decl]
    assert text.index("int inr_mix_apply(") > decl
    assert len(L.SYMBOLS["inr_mix_loss_grad"][1]) == 11 and len(L.SYMBOLS["inr_mix_apply"][1]) == 5
    lib = L.load()
    assert lib.inr_mix_loss_grad is not None and lib.inr_mix_apply is not None
    for name, val in (("INR_MIX_MAX_HEADS", L.MIX_MAX_HEADS), ("INR_MIX_BLOCKS", L.MIX_BLOCKS),
                      ("INR_MIX_PARTIALS", L.MIX_PARTIALS)):
        assert f"#define {name} {val}\n" in text
    assert L.MIX_PARTIALS + (L.MIX_MAX_HEADS + 1) * L.MIX_BLOCKS <= L.LOSS_WORDS
    import ctypes as Ct
    assert Ct.sizeof(L.MixDesc) == 16 + 36 + 36 + 64 + 64  # no padding: 88 bytes in front of the pointer tables
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        assert "inr_mix.hip" in f.read()


def test_bindings_refuse_host_tensors_and_bad_shapes():
    ys, w, gt, d = [torch.zeros(4, 2)] * 2, torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.mix_apply(ys, w)
    with pytest.raises(RuntimeError, match="shape"):
        M.mix_apply(ys, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="shape"):
        M.mix_loss_grad(_spec("l2"), ys, w, gt, torch.zeros(5), [0.0, 1.0, 2.0], [0.25] * 3)
    with pytest.raises(ValueError, match="2..8"):
        M.mix_apply([torch.zeros(4, 2)], torch.zeros(4, 1))
    with pytest.raises(ValueError, match="increase"):
        M.check_radii([0.0, 1.0, 1.0], 2)


def test_command_line_and_config(tmp_path):
    from inr_mi355x.cli import get_config, parse_cli
    from inr_mi355x.train_multihead import check_mixture_config, mixture_heads, mixture_settings
    from inr_mi355x.trainer_base import set_default_configs
    path = os.path.join(ROOT, "configs", "config_siren_multihead.yaml")
    opts, config = parse_cli(argv=["--config", path, "--synthetic", "3,16,12", "--val", "--band-report", "10", "--shuffle"])
    assert opts.val and config["partition"]["no_models"] == 4 and mixture_heads(config) == 4
    check_mixture_config(set_default_configs(dict(config)))
    assert mixture_settings(get_config(path)) == dict(detach=True, clamp=True,
                                                      gate=dict(network_width=128, network_depth=5))
