"""Ring-normalised fits, the part that needs no GPU: ringnorm.ring_scale_numpy against arrays
the reference's own scale_space produced (tests/golden/ring_norm.npz, tools/make_golden_ring_norm.py), the edge rules of
the definition, the table against clustering.partition_and_stats, the checkpoint entry, the refusals, the ABI entry and
the wrapper's argument errors."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from inr_mi355x import _lib as L
from inr_mi355x import ringnorm as R
from inr_mi355x.synthetic import make_kspace

CASES = ("probe", "rings64", "ring1")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "ring_norm.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", CASES)
def test_numpy_equals_reference_bit_for_bit(golden, tag):
    g = lambda k: golden[f"{tag}/{k}"]
    values = g("values").copy()
    fwd = R.ring_scale_numpy(g("dist"), values, g("radii"), g("divisors"))
    assert fwd.dtype == np.float32 and np.array_equal(_bits(fwd), _bits(g("forward")))
    assert np.array_equal(_bits(values), _bits(g("values")))  # the input is not modified
    inv = R.ring_scale_numpy(g("dist"), fwd, g("radii"), R.inverse_divisors(g("divisors")))
    assert np.array_equal(_bits(inv), _bits(g("inverse")))
    # CPU tensors are taken as well
    assert np.array_equal(_bits(R.ring_scale_numpy(torch.from_numpy(g("dist")), torch.from_numpy(values), g("radii"),
                                                   g("divisors"))), _bits(fwd))


def test_boundary_outside_and_nan_rows():
    radii = np.array([0.25, 0.5, 0.5, 1.0])  # ring 1 is empty
    div = np.array([2.0, 3.0, 5.0], dtype=np.float32)
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    dist = np.array([0.25, below(0.25), 0.5, below(0.5), below(1.0), 1.0, 7.0, np.nan, -1.0, 0.0], dtype=np.float32)
    v = np.stack([np.arange(1, 11), -np.arange(1, 11) * 0.5], axis=1).astype(np.float32)
    v[7] = [np.float32(np.nan), -0.0]  # a NaN-dist row with a NaN payload and a negative zero: copied bit for bit
    out = R.ring_scale_numpy(dist, v, radii, div)
    ring = [0, None, 2, 0, 2, None, None, None, None, None]  # 0.5 itself: past the empty ring, into ring 2
    for i, r in enumerate(ring):
        want = v[i] if r is None else (v[i] / div[r]).astype(np.float32)
        assert np.array_equal(_bits(out[i]), _bits(want)), (i, out[i], want)
    # radii are rounded to fp32 before they are compared: fl32(0.7) lies BELOW the fp64 0.7, and a row there is still
    # inside a ring that starts at 0.7 and outside one that ends there
    d32 = np.array([np.float32(0.7)], dtype=np.float32)
    assert np.float64(d32[0]) < 0.7
    out = R.ring_scale_numpy(d32, np.ones((1, 2), np.float32), [0.7, 1.0], [4.0])
    assert out.tolist() == [[0.25, 0.25]]
    out = R.ring_scale_numpy(d32, np.ones((1, 2), np.float32), [0.0, 0.7], [4.0])
    assert out.tolist() == [[1.0, 1.0]]


@pytest.mark.parametrize("tag", CASES)
def test_inverse_of_forward_is_within_two_roundings(golden, tag):
    g = lambda k: golden[f"{tag}/{k}"]
    v, dist, radii, div = g("values"), g("dist"), g("radii"), g("divisors")
    fwd = R.ring_scale_numpy(dist, v, radii, div)
    inv = R.ring_scale_numpy(dist, fwd, radii, R.inverse_divisors(div))
    rel = np.abs(inv.astype(np.float64) - v.astype(np.float64)) / np.abs(v.astype(np.float64))
    print("%s: max relative round-trip error %.4g" % (tag, rel.max()))
    assert rel.max() <= 2.0 ** -22
    r32 = radii.astype(np.float32)
    outside = ~((dist >= r32[0]) & (dist < r32[-1]))
    assert outside.any() or tag == "rings64"
    assert np.array_equal(_bits(fwd[outside]), _bits(v[outside])) and np.array_equal(_bits(inv[outside]), _bits(v[outside]))


@pytest.mark.parametrize("stat", ["max", "min"])
def test_from_rows_equals_partition_and_stats(stat):
    from inr_mi355x.clustering import partition_and_stats
    image, coords, (C, H, W) = make_kspace(2, 16, 12)
    want_stats, want_radii = partition_and_stats(image.reshape(C, H, W, 2), coords.reshape(C, H, W, 3), 10, 3, stat)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    t = R.RingTable.from_rows(image, dist, no_steps=10, no_models=3, stat=stat)
    assert np.array_equal(t.radii, np.asarray(want_radii, dtype=np.float64)) and t.radii.dtype == np.float64
    assert np.array_equal(_bits(t.divisors), _bits(want_stats.numpy())) and t.divisors.dtype == np.float32
    assert (t.stat, t.no_steps, t.no_models, t.rings) == (stat, 10, 3, 3)
    s = t.summary()
    assert set(s) == {"stat", "rings", "radii", "divisors"} and s["rings"] == 3 and len(s["radii"]) == 4
    with pytest.raises(ValueError):
        R.RingTable.from_rows(image, dist, stat="mean")


def test_same_table_and_state_round_trip(tmp_path):
    t = R.RingTable([0.0, 0.3, 0.9, 5.0], np.array([4.0, 0.5, 0.01], np.float32), "max", 40, 4)
    st = t.state()
    assert set(st) == {"radii", "divisors", "stat", "no_steps", "no_models"}
    path = tmp_path / "ckpt.pt"
    torch.save({"ring_normalization": st}, path)
    back = R.RingTable.from_state(torch.load(path)["ring_normalization"])
    assert np.array_equal(back.radii, t.radii) and np.array_equal(_bits(back.divisors), _bits(t.divisors))
    assert (back.stat, back.no_steps, back.no_models) == ("max", 40, 4)
    assert R.same_table(st, back.state()) is None and R.same_table(None, None) is None
    assert "one side" in R.same_table(st, None) and "one side" in R.same_table(None, st)
    other = R.RingTable([0.0, 0.3, 0.9, 5.0], np.array([4.0, 0.5, 0.02], np.float32), "max")
    assert "divisors" in R.same_table(st, other.state())
    other = R.RingTable([0.0, 0.31, 0.9, 5.0], t.divisors, "max")
    assert "radii" in R.same_table(st, other.state())
    assert "rings" in R.same_table(st, R.RingTable([0.0, 5.0], [1.0], "file").state())
    # a file table
    np.savez(tmp_path / "t.npz", radii=t.radii, divisors=t.divisors)
    f = R.RingTable.from_file(str(tmp_path / "t.npz"))
    assert f.stat == "file" and R.same_table(f.state(), st) is None
    np.savez(tmp_path / "bad.npz", radii=t.radii)
    with pytest.raises(ValueError, match="divisors"):
        R.RingTable.from_file(str(tmp_path / "bad.npz"))
    assert np.array_equal(_bits(t.inverse), _bits(np.float32(1.0) / t.divisors))


def test_bad_tables_are_refused():
    d, v = np.zeros(3, np.float32), np.ones((3, 2), np.float32)
    for radii, div in (([0.0, 1.0], []), ([0.0, 1.0, 2.0], [1.0]), ([0.0, np.nan], [1.0]), ([1.0, 0.5], [1.0]),
                       ([0.0, 1.0], [0.0]), ([0.0, 1.0], [np.inf]), ([0.0, 1.0], [np.nan]),
                       (np.arange(66), np.ones(65))):
        with pytest.raises(ValueError):
            R.ring_scale_numpy(d, v, radii, div)
    with pytest.raises(ValueError, match="rows"):
        R.ring_scale_numpy(np.zeros(2, np.float32), v, [0.0, 1.0], [1.0])


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=100, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               ring_normalization="max")
    cfg.update(kw)
    return cfg


def test_trainers_refuse_before_any_device_call():
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    from inr_mi355x.trainer_base import ResidentFit, set_default_configs
    assert "ring_normalization" not in set_default_configs({})  # read with .get: the default key set stays what it was
    image, coords, shape = make_kspace(2, 8, 8)
    mask = torch.ones(2 * 8 * 8, 1, dtype=torch.bool)
    cases = [(dict(transform=True), {}, ValueError), (dict(undersampling="radial-4"), {}, ValueError),
             (dict(undersampling="grid-2*2"), {}, ValueError), ({}, dict(mask=mask), ValueError),
             (dict(ring_normalization="median"), {}, ValueError), (dict(ring_normalization="table.txt"), {}, ValueError)]
    for cfg_kw, ctor_kw, exc in cases:
        with pytest.raises(exc, match="ring_normalization"):
            INRTrainer(_cfg(**cfg_kw), image, coords, shape, "cuda:0", **ctor_kw)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    with pytest.raises(NotImplementedError, match="ring_normalization"):
        MultiscaleTrainer(_cfg(), image, coords, dist, None, shape, "cuda:0")
    with pytest.raises(NotImplementedError, match="ring_normalization"):
        RingEnsembleTrainer(_cfg(), image, coords, shape, "cuda:0")
    # off: absent, None and "none" all mean no table
    fit = ResidentFit()
    for cfg in ({}, {"ring_normalization": None}, {"ring_normalization": "none"}):
        fit._init_fit(cfg, (2, 8, 8), "cpu", 0, 0, 1, None)
        assert fit.ring_norm_spec is None and fit.ring_table is None
    fit._init_fit({"ring_normalization": "min"}, (2, 8, 8), "cpu", 0, 0, 1, None, ring_norm_ok=True)
    assert fit.ring_norm_spec == "min" and fit.ring_table is None
    assert R.partition_counts({}) == (40, 4) and R.partition_counts({"partition": {"no_steps": 12, "no_models": 3}}) == (12, 3)


def test_command_line_flag(tmp_path):
    from inr_mi355x.cli import parse_cli
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model: SIREN\nnormalization: max\n")
    opts, config = parse_cli(argv=["--config", str(cfg)])
    assert opts.ring_normalize is None and "ring_normalization" not in config
    opts, config = parse_cli(argv=["--config", str(cfg), "--ring-normalize", "min"])
    assert config["ring_normalization"] == "min"
    cfg.write_text("model: SIREN\nring_normalization: max\n")
    assert parse_cli(argv=["--config", str(cfg)])[1]["ring_normalization"] == "max"
    assert parse_cli(argv=["--config", str(cfg), "--ring-normalize", "t.npz"])[1]["ring_normalization"] == "t.npz"


def test_header_binding_and_export():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_ring_scale\(const float\* dist, const float\* in, float\* out, int64_t n, const float\* radii, "
                     r"const float\* divisors,\s+int32_t n_rings, void\* stream\);", text, re.M)
    head = text[:text.index("#define INR_ABI_VERSION")]
    assert "inr_ring_scale" in head[head.index("v7 additions"):]  # listed under the v7 additions; the version stays
    assert "#define INR_ABI_VERSION 7\n" in text and L.ABI_VERSION == 7
    decl = text.index("int inr_ring_scale(")
    assert "(v7 addition)" in text[text.rindex("/*", 0, decl):decl]
    assert "inr_ring_scale" in L.SYMBOLS and len(L.SYMBOLS["inr_ring_scale"][1]) == 8
    assert hasattr(L.load(), "inr_ring_scale")  # the built library exports it
    with open(os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc", "Makefile")) as f:
        assert "inr_ring_scale.hip" in f.read()


def test_wrapper_argument_errors_raise_before_any_call():
    radii, div = [0.0, 1.0], [2.0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.ring_scale(torch.zeros(4), torch.zeros(4, 2), radii, div)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.ring_scale(np.zeros(4, np.float32), torch.zeros(4, 2), radii, div)

    class Fake(torch.Tensor):  # passes for a device tensor without a device: what follows must raise before any call
        is_cuda = True

    fake = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).as_subclass(Fake)
    with pytest.raises(RuntimeError, match="float32"):
        R.ring_scale(fake(4, dt=torch.float64), fake(4, 2), radii, div)
    with pytest.raises(RuntimeError, match="float32"):
        R.ring_scale(fake(4), fake(4, 2, dt=torch.float16), radii, div)
    with pytest.raises(RuntimeError, match="rows"):
        R.ring_scale(fake(4), fake(5, 2), radii, div)
    with pytest.raises(RuntimeError, match=r"\[n,2\]"):
        R.ring_scale(fake(4), fake(4, 3), radii, div)
    with pytest.raises(RuntimeError, match="contiguous"):
        R.ring_scale(fake(4), fake(4, 4)[:, :2], radii, div)
    with pytest.raises(RuntimeError, match="rows"):
        R.ring_scale(fake(4), fake(4, 2), radii, div, out=fake(3, 2))
    with pytest.raises(ValueError):
        R.ring_scale(fake(4), fake(4, 2), [1.0, 0.0], div)
