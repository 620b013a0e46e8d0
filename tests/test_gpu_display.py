"""The display kernels on the MI355X (inr_kspace_display, inr_gray8, inr_coil_stats) against the float64 restatement of
tests/test_display.py and the reference's own outputs (tests/golden/display.npz), their call conventions, and the
trainers / CLIs that write the validation epoch's pictures with them.

Tolerance of the continuous outputs: the largest absolute difference between the reference's fp32 arithmetic (the five
lines of save_im and Normalize's two, evaluated by torch on the CPU) and the float64 restatement, measured here over
the fixture and every shape below; the device is allowed four times that (its expm1 / log1p and summation order differ
from torch's by an ulp or two per operation, on values of order one).  Both numbers are recorded through
conftest.record_parity (profiles/display_parity.jsonl is a committed copy of this module's lines)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT, record_parity
from test_display import (CASES, assert_bytes, case_n64, coil_stats64, gray_bytes64, gray_norm64, kspace_display64)

pytestmark = pytest.mark.gpu

SHAPES = [(640, 368), (321, 203), (7, 7), (64, 1000)]
COILS = [1, 15, 32]
U64 = 2.0 ** -52


def record(test: str, **values) -> None:
    record_parity("display/" + test, **{k: float(v) for k, v in values.items()})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "display.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _coils(kind: str, C: int, H: int, W: int):
    """(coils, second) [C,H,W,2] fp32 on the CPU"""
    if kind == "zero":
        return torch.zeros(C, H, W, 2), torch.zeros(C, H, W, 2)
    g = torch.Generator().manual_seed(C * 7 + H)
    if kind == "random":
        return torch.rand(C, H, W, 2, generator=g) - 0.5, torch.rand(C, H, W, 2, generator=g) - 0.5
    from inr_mi355x.synthetic import make_kspace
    image, _, _ = make_kspace(C, H, W, seed=C * 7 + H)
    gt = image.reshape(C, H, W, 2)
    return gt, gt + 0.01 * gt.abs().max() * torch.randn(gt.shape, generator=g)


def torch32_display(coils: torch.Tensor, minus=None, sf: float = 8.0) -> torch.Tensor:
    """models/utils.py:262-267 with torch on the CPU in fp32, as the reference evaluates it"""
    z = coils if minus is None else coils - minus
    g = torch.sqrt((((z ** 2).sum(dim=-1).sqrt()) ** 2).sum(0))
    g = g * (torch.expm1(torch.tensor(sf, dtype=torch.float32)) / g.max())
    g = torch.log1p(g)
    return g / g.max()


def torch32_norm(x: torch.Tensor, take_abs=False, vmin=None, vmax=None) -> torch.Tensor:
    """Normalize's arithmetic on an fp32 picture: (x - vmin) / (vmax - vmin)"""
    x = x.abs() if take_abs else x
    if not (vmin and vmax):
        vmin, vmax = x.min(), x.max()
    return torch.zeros_like(x) if float(vmax) == float(vmin) else (x - vmin) / (vmax - vmin)


_CACHE = {}


def _case(kind, C, H, W):
    """inputs and their float64 / torch-fp32 pictures, computed once per shape"""
    key = (kind, C, H, W)
    if key not in _CACHE:
        a, b = _coils(kind, C, H, W)
        out = {"a": a, "b": b}
        for tag, minus in (("plain", None), ("error", b)):
            d64 = kspace_display64(a.numpy(), None if minus is None else minus.numpy())
            n64 = gray_norm64(d64)
            out[tag] = (d64, n64)
            if kind != "zero":
                d32 = torch32_display(a, minus)
                out[tag + "_t32"] = max(float(np.abs(d32.double().numpy() - d64).max()),
                                        float(np.abs(torch32_norm(d32).double().numpy() - n64).max()))
        if len(_CACHE) > 4:  # keep the host's memory flat: the big shapes are 60 MB each in float64
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = out
    return _CACHE[key]


@pytest.fixture(scope="module")
def tol(gold):
    """max |reference fp32 - float64| over the fixture and over every shape and kind: the measured yardstick"""
    worst = 0.0
    for tag in CASES:
        disp, n = case_n64(gold, tag)
        if disp is not None:
            worst = max(worst, float(np.abs(gold[tag + "/handed"].astype(np.float64) - disp).max()))
        worst = max(worst, float(np.nanmax(np.abs(gold[tag + "/normalized"].astype(np.float64) - n))))
    for kind in ("random", "mri"):
        for C in COILS:
            for (H, W) in SHAPES:
                c = _case(kind, C, H, W)
                worst = max(worst, c["plain_t32"], c["error_t32"])
                x = c["a"][0, :, :, 0]  # a signed picture through np.abs and its own extrema
                n64 = gray_norm64(x.numpy(), True)
                worst = max(worst, float(np.abs(torch32_norm(x, True).double().numpy() - n64).max()))
    _CACHE.clear()
    record("tolerance", reference_fp32_vs_f64=worst, device_allowed=4 * worst)
    assert 0.0 < worst < 1e-5  # sanity of the yardstick itself: a handful of fp32 roundings on values in 0..1
    return 4 * worst


# ---- kernels against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("C", COILS)
@pytest.mark.parametrize("HW", SHAPES)
@pytest.mark.parametrize("kind", ["random", "mri", "zero"])
def test_display_and_bytes_against_restatement(dev, gold, tol, C, HW, kind):
    from inr_mi355x import display as D
    H, W = HW
    c = _case(kind, C, H, W)
    a, b = c["a"].to(dev), c["b"].to(dev)
    lut = gold["lut"]
    worst_d = worst_n = 0.0
    flips = 0
    for tag, minus in (("plain", None), ("error", b)):
        d64, n64 = c[tag]
        disp = D.kspace_display(a, minus)
        norm = torch.empty(H, W, device=dev)
        u8 = D.gray8(disp, norm_out=norm).cpu().numpy()
        got_d, got_n = disp.cpu().double().numpy(), norm.cpu().double().numpy()
        if kind == "zero":  # 0 * (expm1(sf) / 0): NaN everywhere, as the reference; matplotlib masks them -> byte 0
            assert np.isnan(got_d).all() and np.isnan(d64).all() and np.isnan(got_n).all() and not u8.any()
            continue
        dd, dn = float(np.abs(got_d - d64).max()), float(np.abs(got_n - n64).max())
        print(f"[{kind},{C},{H}x{W},{tag}] |display - f64| {dd:.3e}  |n - f64| {dn:.3e}  (allowed {tol:.3e})")
        worst_d, worst_n = max(worst_d, dd), max(worst_n, dn)
        assert dd <= tol and dn <= tol, (tag, dd, dn, tol)
        assert float(got_d.max()) == 1.0 and float(got_d.min()) >= 0.0
        flips += assert_bytes(u8, n64, lut, tol, tag)
    # a signed picture (np.abs, own extrema), a range, and a constant picture straight through inr_gray8
    x = c["a"][0, :, :, 0].contiguous()
    xd = x.to(dev)
    norm = torch.empty(H, W, device=dev)
    for kw in (dict(take_abs=True), dict(take_abs=True, vmin=0.05, vmax=0.3), dict(take_abs=False, vmin=0.0, vmax=0.3)):
        u8 = D.gray8(xd, norm_out=norm, **kw).cpu().numpy()
        n64 = gray_norm64(x.numpy(), kw["take_abs"], kw.get("vmin"), kw.get("vmax"))
        dn = float(np.abs(norm.cpu().double().numpy() - n64).max())
        print(f"[{kind},{C},{H}x{W},gray8 {kw}] |n - f64| {dn:.3e}")
        worst_n = max(worst_n, dn)
        assert dn <= tol, (kw, dn, tol)
        flips += assert_bytes(u8, n64, lut, tol, str(kw))
    record(f"display[{kind},{C},{H}x{W}]", display_vs_f64=worst_d, n_vs_f64=worst_n, allowed=tol, one_step_pixels=flips)


@pytest.mark.parametrize("tag", list(CASES))
def test_fixture_cases_against_the_references_png(dev, gold, tol, tag):
    from inr_mi355x import display as D
    key, minus, is_kspace, take_abs, ranged = CASES[tag]
    disp64, n64 = case_n64(gold, tag)
    lut = gold["lut"]
    if is_kspace:
        m = None if minus is None else torch.from_numpy(gold[minus]).to(dev)
        img = D.kspace_display(torch.from_numpy(gold[key]).to(dev), m, float(gold["smoothing_factor"]))
        dd = float(np.abs(img.cpu().double().numpy() - disp64).max())
        ref_d = float(np.abs(gold[tag + "/handed"].astype(np.float64) - disp64).max())
        record(f"fixture[{tag}]", display_vs_f64=dd, reference_fp32_vs_f64=ref_d, allowed=tol)
        assert dd <= tol, (dd, tol)
        kw = {}
    else:
        img = torch.from_numpy(gold[key]).to(dev)
        lo, hi = (float(v) for v in gold["ranged_vmin_vmax"]) if ranged else (None, None)
        kw = dict(take_abs=take_abs, vmin=lo, vmax=hi)
    norm = torch.empty_like(img)
    u8 = D.gray8(img, norm_out=norm, **kw).cpu().numpy()
    dn = float(np.abs(norm.cpu().double().numpy() - n64).max())
    print(f"{tag}: |n - f64| {dn:.3e} (allowed {tol:.3e})")
    assert dn <= tol
    assert_bytes(u8, n64, lut, tol, tag)
    # and against the bytes the reference's PNG holds, under the same rule: where the two differ, both sit within one
    # index step of the restatement at a pixel whose 256 n is an integer within the tolerance
    ref = gold[tag + "/bytes"]
    assert_bytes(ref, n64, lut, tol, tag + " reference")
    differ = u8 != ref
    print(f"{tag}: {int(differ.sum())} of {ref.size} bytes differ from the reference's PNG")
    if differ.any():
        t = n64 * 256.0
        assert (np.abs(t - np.rint(t)) <= 256.0 * tol)[differ].all()
    if tag == "constant_case":
        assert not u8.any()


@pytest.mark.parametrize("C", COILS)
@pytest.mark.parametrize("HW", SHAPES)
@pytest.mark.parametrize("kind", ["random", "mri", "zero"])
def test_coil_stats_against_float64(dev, C, HW, kind):
    from inr_mi355x import display as D
    H, W = HW
    a, _ = _coils(kind, C, H, W)
    got = D.coil_stats(a.to(dev)).cpu().numpy()
    want = coil_stats64(a.numpy())
    n = 2 * H * W
    mean_abs = np.abs(a.double().numpy()).reshape(C, -1).mean(1)
    # fp64 accumulation of n terms: within n 2^-52 sum|x| of the exact sum -> n 2^-52 mean|x| on the mean; the squared
    # deviations are accumulated the same way (relative n 2^-52 on their sum, half of it on the root), the error of the
    # mean enters them only at second order
    e_mean = np.abs(got[:, 0] - want[:, 0])
    e_std = np.abs(got[:, 1] - want[:, 1])
    record(f"coil_stats[{kind},{C},{H}x{W}]", mean_err=e_mean.max(), mean_bound=(n * U64 * mean_abs).max(),
           std_rel_err=(e_std / np.maximum(want[:, 1], 1e-300)).max(), std_rel_bound=n * U64)
    assert (e_mean <= n * U64 * mean_abs).all(), (e_mean, n * U64 * mean_abs)
    assert (e_std <= n * U64 * want[:, 1]).all(), (e_std, n * U64 * want[:, 1])
    assert np.array_equal(got[:, 2:], want[:, 2:])


def test_coil_stats_against_the_references_numbers(dev, gold):
    from inr_mi355x import display as D
    k = gold["kspace"]
    got = D.coil_stats(torch.from_numpy(k).to(dev)).cpu().numpy()
    ref, want = gold["coil_stats"], coil_stats64(k)  # the reference's fp32 torch numbers; float64 numpy
    measured = np.abs(ref - want).max(0)  # fp32 torch against float64, per column, here on the CPU
    n = k[0].size
    bound = n * U64 * np.array([np.abs(k).mean(), want[:, 1].max(), 0.0, 0.0])
    err = np.abs(got - ref).max(0)
    record("coil_stats[fixture]", **{f"{c}_ref_vs_f64": m for c, m in zip(("mean", "std", "max", "min"), measured)},
           **{f"{c}_dev_vs_ref": e for c, e in zip(("mean", "std", "max", "min"), err)})
    assert (err <= measured + bound).all(), (err, measured, bound)
    assert np.array_equal(got[:, 2:], ref[:, 2:])


# ---- call conventions -----------------------------------------------------------------------------------------------
def test_bitwise_reproducible_allocation_free_and_capturable(dev):
    from inr_mi355x import display as D
    C, H, W = 15, 321, 203
    a, b = (t.to(dev) for t in _coils("mri", C, H, W))
    disp, err = torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
    u8, u8r = (torch.empty(H, W, device=dev, dtype=torch.uint8) for _ in range(2))
    norm = torch.empty(H, W, device=dev)
    stats = torch.empty(C, 4, device=dev, dtype=torch.float64)
    fs = torch.empty(max(D.kspace_display_scratch_floats(C, H, W), D.gray8_scratch_floats(H, W)), device=dev)
    ds = torch.empty(D.coil_stats_scratch_doubles(C, H, W), device=dev, dtype=torch.float64)

    def run():
        D.kspace_display(a, None, out=disp, scratch=fs)
        D.gray8(disp, out=u8, scratch=fs, norm_out=norm)
        D.kspace_display(a, b, out=err, scratch=fs)
        D.gray8(err, vmin=0.1, vmax=0.9, out=u8r)
        D.coil_stats(a, stats, ds)

    def snapshot():
        return [t.clone() for t in (disp.view(torch.int32), err.view(torch.int32), u8, u8r, norm.view(torch.int32),
                                    stats.view(torch.int64))]

    run()  # (first call: uploads the table)
    first = snapshot()
    torch.cuda.synchronize()
    n_alloc = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    run()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n_alloc
    assert all(torch.equal(x, y) for x, y in zip(snapshot(), first))
    for t in (disp, err, u8, u8r, norm, stats):
        t.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run()
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(snapshot(), first))


def test_bad_arguments_raise_with_the_librarys_message(dev):
    from inr_mi355x import display as D
    a = torch.rand(3, 16, 12, 2, device=dev)
    img = torch.rand(16, 12, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.kspace_display(a.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.kspace_display(a, a.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.gray8(img.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.coil_stats(a.cpu())
    with pytest.raises(RuntimeError, match="must be a contiguous torch.float32"):
        D.kspace_display(a.double())
    with pytest.raises(RuntimeError, match="must be a contiguous torch.float32"):
        D.coil_stats(a.double())
    with pytest.raises(RuntimeError, match="must be a contiguous torch.float32"):
        D.gray8(torch.rand(12, 16, device=dev).t())
    with pytest.raises(RuntimeError, match=r"expected \[C,H,W,2\]"):
        D.kspace_display(a[..., 0])
    with pytest.raises(RuntimeError, match="minus has shape"):
        D.kspace_display(a, a[:2].contiguous())
    with pytest.raises(RuntimeError, match=r"expected \[H,W\]"):
        D.gray8(a)
    with pytest.raises(RuntimeError, match="out has shape"):
        D.gray8(img, out=torch.empty(12, 16, device=dev, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="must be a contiguous torch.uint8"):
        D.gray8(img, out=torch.empty(16, 12, device=dev))
    with pytest.raises(RuntimeError, match="must be a contiguous torch.float64"):
        D.coil_stats(a, stats=torch.empty(3, 4, device=dev))
    with pytest.raises(RuntimeError, match="inr_kspace_display: scratch holds 1 floats, needs"):
        D.kspace_display(a, scratch=torch.empty(1, device=dev))
    with pytest.raises(RuntimeError, match="inr_gray8: scratch holds 1 floats, needs"):
        D.gray8(img, scratch=torch.empty(1, device=dev))
    with pytest.raises(RuntimeError, match="inr_coil_stats: scratch holds 2 doubles, needs"):
        D.coil_stats(a, scratch=torch.empty(2, device=dev, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="inr_gray8: minvalue must be less than or equal to maxvalue"):
        D.gray8(img, vmin=0.9, vmax=0.1)


# ---- trainers -------------------------------------------------------------------------------------------------------
def _siren_cfg():
    return dict(model="SIREN", loss="L2", lr=1e-4, batch_size=600, max_epoch=3, weight_decay=0.0, beta1=0.9,
                beta2=0.999, net=dict(network_input_size=64, network_output_size=2, network_depth=3, network_width=32),
                encoder=dict(embedding="gauss", scale=2, embedding_size=32, coordinates_size=3))


def _check_pictures(tr, rec, directory, C, H, W, kspace=True):
    from inr_mi355x import display as D
    e = rec["epoch"] + 1
    names = (["recon_kspace_%ddB.png" % e, "recon_kspace_%d_error.png" % e] if kspace else []) + \
            ["recon_{}_{:.4g}_psnr_{:.4g}_ssim.png".format(e, rec["psnr"], rec["ssim"])]
    assert [os.path.basename(p) for p in rec["images"]] == names
    for p in rec["images"]:
        assert os.path.dirname(p) == str(directory) and D.read_png_gray(p).shape == (H, W)
    assert np.asarray(rec["coil_stats"]).shape == (C, 4)


def test_inr_trainer_writes_the_references_files(dev, tol, tmp_path):
    from inr_mi355x import display as D
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    C, H, W = 2, 40, 30
    image, coords, shape = make_kspace(C, H, W)
    cfg = _siren_cfg()
    plain = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    lp = plain.fit(log_every=1, val_epoch=1)
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    tr.enable_validation_images()
    d = tmp_path / "images"
    train = tr.save_training_images(str(d))
    assert [os.path.basename(p) for p in train] == ["train_kspace.png", "train.png"]
    checked = []

    def on_validate(rec):
        stats = tr.save_validation_images(rec["epoch"], rec, str(d))
        _check_pictures(tr, rec, d, C, H, W)
        # the recon picture is inr_gray8 of the RSS image validate() scored; the k-space pictures are those of the sweep
        rss = tr._metric_bufs[0]
        assert np.array_equal(D.read_png_gray(rec["images"][2]), D.gray8(rss, take_abs=True).cpu().numpy())
        pred = tr.predict_all().reshape(C, H, W, 2)
        full = tr.image_full.reshape(C, H, W, 2)
        assert np.array_equal(D.read_png_gray(rec["images"][0]), D.gray8(D.kspace_display(pred)).cpu().numpy())
        assert np.array_equal(D.read_png_gray(rec["images"][1]), D.gray8(D.kspace_display(pred, full)).cpu().numpy())
        np.testing.assert_allclose(stats.numpy(), coil_stats64(pred.cpu().numpy()), rtol=1e-9, atol=1e-12)
        assert rec["coil_stats"] == stats.tolist()
        checked.append(rec["epoch"])

    lt = tr.fit(log_every=1, val_epoch=1, on_validate=on_validate)
    assert checked == [0, 1, 2] and len(os.listdir(d)) == 2 + 3 * 3
    # pictures change nothing: same losses, same parameters, same records apart from the two new keys
    assert lt == lp and torch.equal(tr.engine.params, plain.engine.params)
    assert [{k: v for k, v in r.items() if k not in ("images", "coil_stats")} for r in tr.val_history] == plain.val_history
    assert all("images" not in r and "coil_stats" not in r for r in plain.val_history)
    assert np.array_equal(D.read_png_gray(train[1]), D.gray8(tr._ref_rss, take_abs=True).cpu().numpy())
    full = tr.image_full.reshape(C, H, W, 2)
    assert np.array_equal(D.read_png_gray(train[0]), D.gray8(D.kspace_display(full)).cpu().numpy())
    # the training picture against the float64 restatement, under the byte rule
    n64 = gray_norm64(kspace_display64(full.cpu().numpy()))
    assert_bytes(D.read_png_gray(train[0]), n64, D.gray_lut(), tol, "train_kspace.png")


def test_save_validation_images_needs_enabling(dev, tmp_path):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 40, 30)
    tr = INRTrainer(_siren_cfg(), image, coords, shape, dev, seed=3)
    rec = tr.validate(0)
    assert tr._last_pred is None and tr._display_bufs is None  # off: nothing kept, no display kernel has run
    with pytest.raises(RuntimeError, match="enable_validation_images"):
        tr.save_validation_images(0, rec, str(tmp_path))


def test_image_space_config_writes_recon_only(dev, tmp_path):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    C, H, W = 2, 40, 30
    image, coords, shape = make_kspace(C, H, W, image_space=True)
    cfg = dict(_siren_cfg(), transform=True, max_epoch=1)
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    tr.enable_validation_images()
    assert [os.path.basename(p) for p in tr.save_training_images(str(tmp_path))] == ["train.png"]
    rec = tr.validate(0)
    tr.save_validation_images(0, rec, str(tmp_path))
    _check_pictures(tr, rec, tmp_path, C, H, W, kspace=False)


def test_multiscale_trainer_writes_pictures(dev, tmp_path):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    C, H, W = 2, 40, 30
    image, coords, shape = make_kspace(C, H, W)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    cfg = dict(model="MultiscaleKFourier", loss="L2", lr=3e-4, batch_size=700, max_epoch=2, weight_decay=0.0,
               beta1=0.9, beta2=0.999,
               net=dict(network_input_size=32, network_output_size=2, network_depth=8, network_width=32),
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3))
    tr = MultiscaleTrainer(cfg, image, coords, dist, [0.0, 0.3, 0.6, 1.0, 1.5], shape, dev, seed=0)
    tr.enable_validation_images()
    assert len(tr.save_training_images(str(tmp_path))) == 2
    tr.fit(val_epoch=1, on_validate=lambda rec: tr.save_validation_images(rec["epoch"], rec, str(tmp_path)))
    assert len(tr.val_history) == 2
    for rec in tr.val_history:
        _check_pictures(tr, rec, tmp_path, C, H, W)


def test_ring_ensemble_writes_pictures(dev, tmp_path):
    from inr_mi355x import display as D
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    C, H, W = 2, 40, 32
    image, coords, shape = make_kspace(C, H, W)
    cfg = dict(model="SIREN", loss="L2", lr=2e-4, batch_size=H * W, max_epoch=3, weight_decay=0.0, beta1=0.9,
               beta2=0.999, partition=dict(no_steps=20, no_models=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3))
    tr = RingEnsembleTrainer(cfg, image, coords, shape, dev, seed=5)
    tr.enable_validation_images()
    tr.save_training_images(str(tmp_path))
    tr.fit(4)
    rec = dict(tr.metrics(), epoch=1)
    tr.save_validation_images(1, rec, str(tmp_path))
    _check_pictures(tr, rec, tmp_path, C, H, W)
    assert np.array_equal(D.read_png_gray(rec["images"][2]), D.gray8(tr._metric_bufs[0], take_abs=True).cpu().numpy())


# ---- command lines, each in a fresh child process ---------------------------------------------------------------------
def _run_cli(module, args, timeout=600):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, "-m", module] + [str(a) for a in args], cwd=PKG, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _cli_cfg(tmp_path, **extra):
    import yaml
    cfg = _siren_cfg()
    cfg.update(max_epoch=2, val_epoch=1, image_save_epoch=1, log_iter=1000, transform=False)
    cfg.update(extra)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p


def test_cli_val_save_images(dev, tmp_path):
    p = _cli_cfg(tmp_path)
    base = ["--config", p, "--synthetic", "2,64,48", "--val", "--max_steps", "100"]
    out = tmp_path / "out"
    stdout = _run_cli("inr_mi355x.train", base + ["--output_path", out, "--save-images"])
    assert stdout.count("[Validation Epoch: ") == 2
    assert stdout.count("K-space Reconstruction Statistics Per Coil") == 2
    assert stdout.index("[Validation Epoch: ") < stdout.index("K-space Reconstruction Statistics Per Coil")
    res = json.loads(stdout.strip().splitlines()[-1])
    images = sorted(os.listdir(out / "images"))
    assert "train.png" in images and "train_kspace.png" in images and len(images) == 2 + 2 * 3
    for rec in res["validation"]:
        assert len(rec["images"]) == 3 and all(os.path.exists(q) for q in rec["images"])
        assert np.asarray(rec["coil_stats"]).shape == (2, 4)
    assert sorted(os.listdir(out / "checkpoints")) == ["model_000001.pt", "model_000002.pt", "model_%06d.pt" % res["steps"]]
    assert sorted(os.listdir(out)) == ["checkpoints", "images"]
    # without the flag: today's layout and keys, and the same fit
    out2 = tmp_path / "out2"
    stdout2 = _run_cli("inr_mi355x.train", base + ["--output_path", out2])
    res2 = json.loads(stdout2.strip().splitlines()[-1])
    assert sorted(os.listdir(out2)) == ["model_000001.pt", "model_000002.pt", "model_%06d.pt" % res2["steps"]]
    assert "Statistics Per Coil" not in stdout2 and "Creating directory" not in stdout2
    assert all(set(r) == {"epoch", "test_loss", "psnr", "ssim"} for r in res2["validation"])
    assert [(r["psnr"], r["ssim"], r["test_loss"]) for r in res["validation"]] == \
           [(r["psnr"], r["ssim"], r["test_loss"]) for r in res2["validation"]]
    assert res["psnr"] == res2["psnr"]


def test_cli_save_images_needs_val(dev, tmp_path):
    p = _cli_cfg(tmp_path)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, "-m", "inr_mi355x.train", "--config", str(p), "--synthetic", "2,64,48",
                        "--save-images"], cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--save-images needs --val" in r.stderr


def test_cli_data_samples_runs_one_fit_per_slice(dev, tmp_path):
    import yaml
    rng = np.random.default_rng(0)
    k = (rng.standard_normal((3, 2, 48, 40)) + 1j * rng.standard_normal((3, 2, 48, 40))).astype(np.complex64)
    scans = tmp_path / "scans"
    scans.mkdir()
    np.savez(scans / "scan0.npz", kspace=k, crop_size=np.array([40, 32, 1]))
    p = _cli_cfg(tmp_path, custom_file_or_path=str(scans), normalization="max", max_epoch=1)
    s = tmp_path / "samples.yaml"
    s.write_text(yaml.safe_dump({"samples": {0: [0, 2]}}))
    out = tmp_path / "out"
    stdout = _run_cli("inr_mi355x.train", ["--config", p, "--data_samples", s, "--val", "--save-images",
                                           "--output_path", out, "--max_steps", "20"])
    lines = [json.loads(l) for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and lines[0]["psnr"] != lines[1]["psnr"]  # two different slices
    assert sorted(os.listdir(out)) == ["sample_0_slice_0", "sample_0_slice_2"]
    for sub in os.listdir(out):
        assert sorted(os.listdir(out / sub)) == ["checkpoints", "images"]
        assert "train.png" in os.listdir(out / sub / "images")


def test_cli_multiscale_and_ring_save_images(dev, tmp_path):
    import yaml
    cfg = dict(model="MultiscaleKFourier", loss="L2", lr=3e-4, batch_size=700, max_epoch=1, weight_decay=0.0,
               beta1=0.9, beta2=0.999, val_epoch=1, image_save_epoch=1, log_iter=1000, transform=False,
               partition=dict(no_steps=20, no_models=4),
               net=dict(network_input_size=32, network_output_size=2, network_depth=8, network_width=32),
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3))
    p = tmp_path / "ms.yaml"
    p.write_text(yaml.safe_dump(cfg))
    out = tmp_path / "ms"
    stdout = _run_cli("inr_mi355x.train_kspace_multiscale", ["--config", p, "--synthetic", "2,40,30", "--val",
                                                             "--save-images", "--output_path", out, "--max_steps", "4"])
    res = json.loads(stdout.strip().splitlines()[-1])
    assert len(res["validation"]) == 1 and len(res["validation"][0]["images"]) == 3
    assert len(os.listdir(out / "images")) == 5 and "Statistics Per Coil" in stdout
    ring = dict(_siren_cfg(), partition=dict(no_steps=20, no_models=3), max_epoch=1, log_iter=1000, transform=False)
    q = tmp_path / "ring.yaml"
    q.write_text(yaml.safe_dump(ring))
    out = tmp_path / "ring"
    stdout = _run_cli("inr_mi355x.train_ring_ensemble", ["--config", q, "--synthetic", "2,40,32", "--save-images",
                                                         "--output_path", out, "--max_steps", "4"])
    res = json.loads(stdout.strip().splitlines()[-1])
    assert len(res["images"]) == 3 and all(os.path.exists(i) for i in res["images"]) and 0.0 < res["ssim"] <= 1.0
    assert len(os.listdir(out / "images")) == 5 and sorted(os.listdir(out / "checkpoints")) == [
        "submodel_0.pt", "submodel_1.pt", "submodel_2.pt"]
