"""Learned radial gain without a GPU (inr_mi355x/gain.py, inr_mi355x/train_scaling.py): the float64
statement of inr_gain_loss_grad against torch.autograd on the oracle's loss functions in float64, and against the table
of tests/loss_cases.py the loss kernels are held to; the two C-ABI entries in header, binding and Makefile; every refusal
of ScaledFitTrainer; gain_inputs; the checkpoint's key names against a module built like the reference's ScalerWrapper;
the two cross-loading refusals."""
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as C
import oracle as O
from aux_bits_cases import rnd
from conftest import ROOT

from inr_mi355x import _lib as L
from inr_mi355x import gain as G
from inr_mi355x.engine import LossSpec

OPTS = dict(hdr_eps=C.EPS, hdr_ff_sigma=2.0, hdr_ff_factor=C.FACTOR, min_sample=4)
f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def _spec(kind):
    return LossSpec(C.KINDS[kind], C.EPS, 2.0, C.FACTOR, 3000)


def _oracle(kind, y, t, kc):
    """scale * loss_fn of the reference's loops (train.py:176-182), as tests/test_loss_host.py calls the oracle"""
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


def _inputs(kind, B):
    """y, gt at amplitude 0.3 (msle: positive, and s >= 0 so that res + 1 stays positive), s uniform in [-1, 1]: |res| stays
    below 0.82, where 1 - tanh^2(res) keeps its digits in float64 (at s = -3, tanh(0.3 e^3) = 1 - 1e-5 and the two float64
    evaluations of 1 - tanh^2, here and in autograd, differ by 1e-12 relative already)"""
    y, t = rnd(B * 2, 31, 0.3).reshape(B, 2), rnd(B * 2, 32, 0.3).reshape(B, 2)
    s = rnd(B, 33, 1.0)
    if kind == "msle":
        y, t, s = np.abs(y) + np.float32(0.05), np.abs(t) + np.float32(0.05), np.abs(s)
    return y, s, t


def _close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert np.all(err <= rel * np.abs(want)), (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))


@pytest.mark.parametrize("kind", list(C.KINDS))
def test_numpy_statement_is_autograd_in_float64(kind):
    """loss, res, dy and ds of gain_loss_grad_numpy against torch.autograd of scale * loss_fn(y exp(-s), gt) over the
    masked rows in float64, rtol 1e-12 per element; unsampled rows are exactly 0."""
    for B in (1, 7, 257):
        y, s, t = _inputs(kind, B)
        for tag in ("none", "half", "single"):
            m, _ = C.mask_of(tag, B)
            keep = np.ones(B, dtype=bool) if m is None else m != 0
            count = int(keep.sum())
            kc = np.zeros((count, 3))
            kc[:, 1], kc[:, 2] = (2.0, 0.0) if kind == "center" else (rnd(count, 40, 1.0), rnd(count, 41, 1.0))
            kc = f64(kc)
            A = float(torch.mean((1.0 - torch.exp(-(kc[:, 1] ** 2 + kc[:, 2] ** 2) / (2 * 2.0 ** 2))) ** 2))
            yt, st = f64(y).requires_grad_(True), f64(s).requires_grad_(True)
            res = yt * torch.exp(-st)[:, None]
            sel = torch.from_numpy(keep)
            loss = _oracle(kind, res[sel], f64(t)[sel], kc)
            gy, gs = torch.autograd.grad(loss, (yt, st))
            got = G.gain_loss_grad_numpy(_spec(kind), y, s, t, m, count, A)
            _close(got[0], float(loss.detach()), (kind, B, tag, "loss"))
            _close(got[1], res.detach().numpy(), (kind, B, tag, "res"))
            _close(got[2], gy.numpy(), (kind, B, tag, "dy"))
            _close(got[3], gs.numpy(), (kind, B, tag, "ds"))
            assert not got[2][~keep].any() and not got[3][~keep].any()
            assert got[1].shape == (B, 2) and got[2].shape == (B, 2) and got[3].shape == (B,)


@pytest.mark.parametrize("kind", list(C.KINDS))
def test_loss_rows_are_the_table_of_the_loss_tests(kind):
    """loss_rows_float64 against loss_cases.row_terms over V, the float64 references tests/test_gpu_loss.py holds
    inr_loss_grad to -- on its own rows, edge rows included"""
    y, t, _ = C.rows(kind, 257)
    inv = C.V.const(1.0 / 257)
    Lr, g0, g1 = C.row_terms(C.V, kind, y, t, inv, hdr_A=C.HDR_A)
    got_L, got_g = G.loss_rows_float64(_spec(kind), y, t, 1.0 / 257, C.HDR_A)
    _close(got_L, Lr.x, (kind, "L"), rel=1e-12)
    _close(got_g, np.stack([g0.x, g1.x], axis=1), (kind, "g"), rel=1e-12)


def test_gain_inputs_on_a_grid():
    from inr_mi355x.synthetic import create_coords
    coords = create_coords(2, 4, 6)
    z = G.gain_inputs(coords)
    assert z.shape == (48, 2) and z.dtype == torch.float32 and z.is_contiguous()
    c = coords.numpy()
    assert np.array_equal(z[:, 0].numpy(), c[:, 0])
    want = np.sqrt((c[:, 1] * c[:, 1]).astype(np.float32) + (c[:, 2] * c[:, 2]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(z[:, 1].numpy(), want)
    assert set(np.unique(z[:, 0].numpy())) == {-1.0, 1.0}  # the coil column: one gain curve per coil
    assert float(z[:, 1].max()) == pytest.approx(np.sqrt(2.0), rel=1e-6)
    with pytest.raises(RuntimeError, match="expected"):
        G.gain_inputs(torch.zeros(5, 2))


def test_header_binding_and_makefile():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_gain_loss_grad\(const inr_loss_desc\* loss, const float\* y, const float\* s, "
                     r"const float\* gt, const uint8_t\* mask,\s+int64_t B, float\* res, float\* loss_out, float\* dy, "
                     r"float\* ds, void\* stream\);", text, re.M)
    assert re.search(r"^int inr_gain_apply\(const float\* y, const float\* s, int64_t B, float\* res, void\* stream\);",
                     text, re.M)
    head = text[:text.index("#define INR_ABI_VERSION")]
    for name in ("inr_gain_loss_grad", "inr_gain_apply"):
        assert name in head[head.index("v7 additions"):]  # listed under the v7 additions; the version stays
        assert hasattr(L.load(), name)  # the built library exports it
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7 and L.load().inr_abi_version() == 7
    decl = text.index("int inr_gain_loss_grad(")
    assert "(v7 additions)" in text[text.rindex("/*", 0, decl):decl]
    assert len(L.SYMBOLS["inr_gain_loss_grad"][1]) == 11 and len(L.SYMBOLS["inr_gain_apply"][1]) == 5
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        assert "inr_gain.hip" in f.read()


def test_bindings_refuse_host_tensors_and_bad_shapes():
    y, s, t = torch.zeros(4, 2), torch.zeros(4), torch.zeros(4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.gain_loss_grad(_spec("l2"), y, s, t, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.gain_apply(y, s)
    with pytest.raises(RuntimeError, match="shape"):
        G.gain_loss_grad(_spec("l2"), y, torch.zeros(4, 1), t, 4)
    with pytest.raises(RuntimeError, match="shape"):
        G.gain_loss_grad(_spec("l2"), y, s, torch.zeros(3, 2), 4)
    with pytest.raises(RuntimeError, match="shape"):
        G.gain_apply(torch.zeros(4, 3), s)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=100, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               scaler=dict(network_width=32, network_depth=3))
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
    (dict(regularization=dict(type="L2", strenght=1e-4)), {}, "regularization"),
    (dict(regularization=dict(type="L1", strenght=1e-4)), {}, "regularization"),
    (dict(trajectory="radial-8"), {}, "trajectory"),
    (dict(ring_normalization="max"), {}, "ring_normalization"),
    (dict(row_sampling="ring-inverse"), {}, "row_sampling"),
    ({}, dict(graph_steps=True), "graph_steps"),
    ({}, dict(rank=0, world=2), "one rank"),
]


@pytest.mark.parametrize("cfg_kw, ctor_kw, match", REFUSALS, ids=[r[2] + str(i) for i, r in enumerate(REFUSALS)])
def test_trainer_refuses_before_any_device_call(cfg_kw, ctor_kw, match):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_scaling import ScaledFitTrainer
    image, coords, shape = make_kspace(2, 8, 8)
    with pytest.raises(NotImplementedError, match=match):
        ScaledFitTrainer(_cfg(**cfg_kw), image, coords, shape, "cuda:0", **ctor_kw)


def test_scaler_size_key():
    from inr_mi355x.train_scaling import SCALER_NET, scaler_net
    assert scaler_net({}) == SCALER_NET == dict(network_input_size=2, network_output_size=1, network_depth=8,
                                                network_width=512)  # the reference's (models/networks.py:388-393)
    assert scaler_net({"scaler": {"network_width": 64}}) == dict(SCALER_NET, network_width=64)
    assert scaler_net({"scaler": {"network_width": 64, "network_depth": 3}})["network_depth"] == 3
    with pytest.raises(ValueError, match="scaler"):
        scaler_net({"scaler": {"network_input_size": 3}})
    with pytest.raises(ValueError, match="scaler"):
        scaler_net({"scaler": {"network_depth": 1}})


class _ScalerWrapper(torch.nn.Module):
    """models/networks.py:380-405 restated: the attribute names that make the state_dict keys"""

    def __init__(self, backbone, width=512, depth=8):
        super().__init__()
        self.backbone = backbone
        layers, n_in = [], 2
        for _ in range(depth - 1):  # FFN (models/networks.py:48-69): Linear / ReLU pairs, then Linear / Sigmoid
            layers += [torch.nn.Linear(n_in, width), torch.nn.ReLU()]
            n_in = width
        layers += [torch.nn.Linear(n_in, 1), torch.nn.Sigmoid()]
        ffn = torch.nn.Module()
        ffn.model = torch.nn.Sequential(*layers)
        self.scaler = ffn


def test_checkpoint_keys_are_the_wrappers():
    import inr_mi355x as M
    from inr_mi355x.train_scaling import SCALER_NET, has_scaler_keys, split_state, wrapper_state
    net = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)
    for width, depth in ((512, 8), (64, 3)):
        back = M.SIREN(net)
        got = wrapper_state(back, M.FFN(dict(SCALER_NET, network_width=width, network_depth=depth)))
        ref_back = torch.nn.Module()  # SIREN's keys: model.{k}.linear.weight / .bias (models/networks.py:79,114-117)
        ref_back.model = torch.nn.Sequential(*[_siren_layer(i, o) for i, o in ((32, 32), (32, 32), (32, 2))])
        want = _ScalerWrapper(ref_back, width, depth).state_dict()
        assert list(got.keys()) == list(want.keys())
        assert [tuple(v.shape) for v in got.values()] == [tuple(v.shape) for v in want.values()]
        assert has_scaler_keys(got) and not has_scaler_keys(back.state_dict())
        b, s = split_state(got)
        assert list(b.keys()) == list(back.state_dict().keys()) and list(s.keys())[0] == "model.0.weight"
    with pytest.raises(ValueError, match="outside"):
        split_state({"model.0.weight": torch.zeros(1)})


def _siren_layer(n_in, n_out):
    layer = torch.nn.Module()
    layer.linear = torch.nn.Linear(n_in, n_out)
    return layer


def test_cross_loading_is_refused_by_name():
    import inr_mi355x as M
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_scaling import SCALER_NET, ScaledFitTrainer, wrapper_state
    net = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)
    back = M.SIREN(net)
    scaled = {"net": wrapper_state(back, M.FFN(dict(SCALER_NET, network_width=32, network_depth=3))), "enc": None}
    plain = {"net": back.state_dict(), "enc": None}
    with pytest.raises(ValueError, match=r"inr_mi355x\.train_scaling"):
        INRTrainer.load_checkpoint(object.__new__(INRTrainer), scaled)
    with pytest.raises(ValueError, match=r"inr_mi355x\.train\)"):
        ScaledFitTrainer.load_checkpoint(object.__new__(ScaledFitTrainer), plain)


def test_command_line(tmp_path):
    """the flags of inr_mi355x.train that apply are parsed by the shared parser"""
    from inr_mi355x.cli import parse_cli
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model: SIREN\nscaler: {network_width: 64, network_depth: 3}\n")
    opts, config = parse_cli(argv=["--config", str(cfg), "--synthetic", "2,16,24", "--val", "--save-images", "--shuffle",
                                   "--shuffle-seed", "5", "--band-report", "10", "--virtual-coils", "2", "--output_path",
                                   str(tmp_path)])
    assert config["scaler"] == {"network_width": 64, "network_depth": 3} and config["shuffle"] and opts.val
    import inr_mi355x.train_scaling as T
    assert callable(T.main)
