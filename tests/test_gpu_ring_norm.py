"""Ring-normalised fits on the MI355X (``-m gpu``): inr_ring_scale against
ringnorm.ring_scale_numpy bit for bit (every path of the kernel: whole groups and the partial last one, 16-byte and
scalar access, in place and out of place, one tile and several, nothing written past row n), its refusals, and the
trainer, the checkpoint, ``reconstruct`` and the search on top of it.

The trainer cases use an explicit table file, so they do not depend on k-means.  Every bit-equality between a
normalised fit and a key-off fit on pre-scaled data rests on one condition, asserted on the CPU first: no row's radius
lies within 1e-5 of a radius of the table (the device and the host may differ in the last bit of a radius -- 2^-24
relative -- and a row must not change ring)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import ringnorm as R
from inr_mi355x.synthetic import make_kspace

pytestmark = pytest.mark.gpu

SENTINEL = 777.25
TAIL = 8  # sentinel rows behind row n - 1
SHAPE = (2, 16, 12)
TABLE = dict(radii=np.array([0.0, 0.3137, 0.7741, 5.0]), divisors=np.array([6.5, 0.75, 0.0625 * 1.3], dtype=np.float32))
MARGIN = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel --------------------------------------------------------------------------------------------------------
def _table(K: int):
    """(radii fp64 [K+1], divisors fp32 [K]): the first radius above 0, the last below the largest dist, and -- from four
    rings on -- one empty ring"""
    rng = np.random.default_rng(100 + K)
    radii = 0.05 + 1.15 * np.arange(K + 1) / K
    if K >= 4:
        radii[2] = radii[1]  # ring 1 is empty
    if K >= 64:
        radii[41] = radii[40] = radii[39]  # two empty rings in a row
    return radii, np.exp(rng.uniform(np.log(1e-3), np.log(1e2), K)).astype(np.float32)


def _rows(n: int, radii: np.ndarray):
    """dist [n] and values [n,2]: rows exactly on radii, one fp32 step below them, below the first radius, at and above the
    last, NaN -- the special rows first, so that the smallest n still meet some -- and random rows in between; values are
    normal fp32 numbers whose quotients are normal too"""
    rng = np.random.default_rng(n)
    r32 = radii.astype(np.float32)
    special = np.concatenate([r32[[0, -1, 1]], [np.nan, 0.0, 1.3, np.nextafter(r32[-1], np.float32(0))], r32[2:-1],
                              np.nextafter(r32[:-1], np.float32(0))]).astype(np.float32)
    dist = rng.uniform(0.0, 1.45, n).astype(np.float32)
    k = min(n, special.size)
    dist[:k] = special[:k]
    if n > special.size:  # spread them over the tiles
        dist = dist[rng.permutation(n)]
    values = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 2))) * rng.choice([-1.0, 1.0], (n, 2))).astype(np.float32)
    return dist, values


@pytest.mark.parametrize("K", [1, 4, 64])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_kernel_equals_numpy_bit_for_bit(dev, n, K):
    _check_kernel(dev, n, K)


def test_kernel_grid_stride_beyond_2048_tiles(dev):
    """more tiles of 1024 rows than the kernel launches blocks (2048): every block takes a second tile, some a partial one"""
    _check_kernel(dev, 2048 * 1024 + 1029, 4)


def _check_kernel(dev, n, K):
    radii, div = _table(K)
    dist, values = _rows(n, radii)
    want = torch.from_numpy(R.ring_scale_numpy(dist, values, radii, div))
    inside = (dist >= np.float32(radii[0])) & (dist < np.float32(radii[-1]))
    assert np.array_equal(want.numpy()[~inside].view(np.uint32), values[~inside].view(np.uint32))
    for off in (0, 1):  # 16-byte aligned buffers; views that start one row in (dist 4-byte, in / out 8-byte aligned)
        rows = off + n + TAIL
        d_buf = torch.full((rows,), float("nan"), device=dev)
        d_buf[off:off + n] = torch.from_numpy(dist).to(dev)
        d_buf[off + n:] = float(radii[0])  # rows behind n would be scaled if they were touched
        v_buf = torch.full((rows, 2), SENTINEL, device=dev)
        v_buf[off:off + n] = torch.from_numpy(values).to(dev)
        keep = v_buf.clone()
        d, v = d_buf[off:off + n], v_buf[off:off + n]
        assert d.data_ptr() % 16 == 4 * off and v.data_ptr() % 16 == 8 * off
        # out of place
        o_buf = torch.full((rows, 2), SENTINEL, device=dev)
        got = R.ring_scale(d, v, radii, div, out=o_buf[off:off + n])
        assert got.data_ptr() == o_buf[off:off + n].data_ptr()
        assert _bits_equal(got.cpu(), want), (n, K, off)
        assert _bits_equal(v_buf, keep)  # `in` is unchanged
        assert bool((o_buf[:off] == SENTINEL).all()) and bool((o_buf[off + n:] == SENTINEL).all())
        # two calls give the same bits
        assert _bits_equal(R.ring_scale(d, v, radii, div), got)
        # in place
        assert R.ring_scale(d, v, radii, div, out=v).data_ptr() == v.data_ptr()
        assert _bits_equal(v.cpu(), want), (n, K, off, "in place")
        assert bool((v_buf[:off] == SENTINEL).all()) and bool((v_buf[off + n:] == SENTINEL).all())
        # and back: the same call with the reciprocal table, within two roundings of the input
        back = R.ring_scale(d, v, radii, R.inverse_divisors(div)).cpu()
        assert _bits_equal(back, torch.from_numpy(R.ring_scale_numpy(dist, want, radii, R.inverse_divisors(div))))
        rel = ((back.double() - torch.from_numpy(values).double()).abs() / torch.from_numpy(values).double().abs()).max()
        assert float(rel) <= 2.0 ** -22, float(rel)


def test_refusals_launch_nothing(dev):
    lib = L.load()
    n, K = 64, 3
    FP = ctypes.POINTER(ctypes.c_float)
    dist = torch.rand(n, device=dev)
    vin = torch.ones(n + 2, 2, device=dev)
    out = torch.full((n + 2, 2), SENTINEL, device=dev)
    good = dict(dist=dist.data_ptr(), vin=vin.data_ptr(), out=out.data_ptr(), n=n,
                radii=np.array([0.0, 0.3, 0.6, 2.0], np.float32), div=np.array([2.0, 3.0, 4.0], np.float32), K=K)

    def call(**kw):
        a = dict(good, **kw)
        r = None if a["radii"] is None else np.ascontiguousarray(a["radii"], np.float32)
        d = None if a["div"] is None else np.ascontiguousarray(a["div"], np.float32)
        rc = lib.inr_ring_scale(a["dist"], a["vin"], a["out"], a["n"], None if r is None else r.ctypes.data_as(FP),
                                None if d is None else d.ctypes.data_as(FP), a["K"],
                                torch.cuda.current_stream(dev).cuda_stream)
        return rc, L.last_error()

    nan, inf = float("nan"), float("inf")
    bad = [(dict(dist=None), "null"), (dict(vin=None), "null"), (dict(out=None), "null"), (dict(radii=None), "null"),
           (dict(div=None), "null"), (dict(n=0), "n = 0"), (dict(n=-5), "n = -5"), (dict(n=1 << 31), "n = 2147483648"),
           (dict(K=0), "n_rings"), (dict(K=65), "n_rings"), (dict(K=-1), "n_rings"),
           (dict(radii=[0.0, nan, 0.6, 2.0]), "NaN"), (dict(radii=[nan, 0.3, 0.6, 2.0]), "NaN"),
           (dict(radii=[0.0, 0.3, 0.6, nan]), "NaN"), (dict(radii=[0.0, 0.7, 0.6, 2.0]), "decrease"),
           (dict(div=[2.0, 0.0, 4.0]), "divisors[1]"), (dict(div=[2.0, 3.0, -0.0]), "divisors[2]"),
           (dict(div=[nan, 3.0, 4.0]), "divisors[0]"), (dict(div=[2.0, inf, 4.0]), "divisors[1]"),
           (dict(div=[2.0, 3.0, -inf]), "divisors[2]"),
           (dict(vin=vin.data_ptr() + 4), "aligned"), (dict(out=out.data_ptr() + 4), "aligned"),
           (dict(dist=dist.data_ptr() + 2), "aligned"),
           (dict(vin=out.data_ptr() + 8), "overlaps in"), (dict(vin=out.data_ptr() + 8 * n - 8), "overlaps in"),
           (dict(vin=out.data_ptr() - 8 * n + 8), "overlaps in"),
           (dict(dist=out.data_ptr()), "overlaps dist"), (dict(dist=out.data_ptr() + 8 * n - 4), "overlaps dist")]
    for kw, text in bad:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("inr_ring_scale"), (kw, rc, msg)
    torch.cuda.synchronize(dev)
    assert bool((out == SENTINEL).all()), "a refused call launched"
    # the same arguments, unspoiled, go through: in place included, and equal neighbouring radii
    assert call()[0] == 0 and call(vin=out.data_ptr())[0] == 0 and call(radii=[0.0, 0.3, 0.3, 2.0])[0] == 0
    torch.cuda.synchronize(dev)
    assert bool((out[n:] == SENTINEL).all()) and not bool((out[:n] == SENTINEL).any())


def test_capturable_in_a_graph(dev):
    radii, div = _table(4)
    dist, values = _rows(1025, radii)
    d, v = torch.from_numpy(dist).to(dev), torch.from_numpy(values).to(dev)
    out = torch.zeros_like(v)
    R.ring_scale(d, v, radii, div, out=out)  # loads the library before the capture
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        R.ring_scale(d, v, radii, div, out=out)
    g.replay()
    torch.cuda.synchronize(dev)
    assert _bits_equal(out.cpu(), torch.from_numpy(R.ring_scale_numpy(dist, values, radii, div)))


# ---- the trainer -------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=100, max_epoch=4, weight_decay=0.0, beta1=0.9, beta2=0.999,
               val_epoch=1, encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


def _radius(coords: torch.Tensor) -> np.ndarray:
    c = coords.cpu()
    return torch.sqrt(c[:, 1] ** 2 + c[:, 2] ** 2).numpy()


def _assert_clear_of_the_table(dist: np.ndarray) -> None:
    gap = np.abs(dist.astype(np.float64)[:, None] - TABLE["radii"][None, 1:]).min()
    assert gap > MARGIN, gap
    assert dist.min() >= 0.0 and dist.max() < 5.0


@pytest.fixture(scope="module")
def scan():
    return make_kspace(*SHAPE)


@pytest.fixture(scope="module")
def table_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ring") / "table.npz")
    np.savez(path, **TABLE)
    return path


def _losses(tr, steps):
    return [v for _, v in tr.fit(steps, log_every=1)]


@pytest.fixture(scope="module")
def grid_pair(scan, table_file, dev):
    """(normalised trainer, key-off trainer on data pre-scaled by ring_scale_numpy, their losses) after six steps"""
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    dist = _radius(coords)
    _assert_clear_of_the_table(dist)
    pre = torch.from_numpy(R.ring_scale_numpy(dist, image, **TABLE))
    a = INRTrainer(_cfg(ring_normalization=table_file), image, coords, shape, dev, seed=3)
    b = INRTrainer(_cfg(), pre, coords, shape, dev, seed=3)
    return a, b, _losses(a, 6), _losses(b, 6)


def test_fit_equals_key_off_fit_on_prescaled_data(scan, grid_pair, dev):
    a, b, la, lb = grid_pair
    image = scan[0]
    assert len(la) == 6 and la == lb, (la, lb)
    assert _bits_equal(a.engine.params, b.engine.params)
    # the trainer scaled into a buffer of its own: the resident data and the caller's tensor are what they were
    assert _bits_equal(a.image_full.cpu(), image) and a.train_values.data_ptr() != a.image_full.data_ptr()
    assert a.image is a.image_full and _bits_equal(a.train_values, b.image_full)
    assert a.ring_table.stat == "file" and a.ring_table.rings == 3 and b.ring_table is None


def test_graph_steps_fit_equals_key_off_fit_on_prescaled_data(scan, table_file, dev):
    """the captured steps read fixed views of the trainer's own scaled buffer"""
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    pre = torch.from_numpy(R.ring_scale_numpy(_radius(coords), image, **TABLE))
    a = INRTrainer(_cfg(ring_normalization=table_file), image, coords, shape, dev, seed=3, graph_steps=True)
    b = INRTrainer(_cfg(), pre, coords, shape, dev, seed=3, graph_steps=True)
    assert a.graph_steps and b.graph_steps
    la, lb = _losses(a, 6), _losses(b, 6)
    assert len(la) == 6 and la == lb, (la, lb)
    assert _bits_equal(a.engine.params, b.engine.params)


def test_validation_scores_in_data_units(scan, grid_pair, dev):
    from inr_mi355x.train import INRTrainer
    a, b, _, _ = grid_pair
    image, coords, shape = scan
    raw = a._predict_raw()
    assert _bits_equal(raw, b.predict_all())
    unscaled = torch.from_numpy(R.ring_scale_numpy(_radius(coords), raw.cpu(), TABLE["radii"],
                                                   R.inverse_divisors(TABLE["divisors"])))
    assert _bits_equal(a.predict_all().cpu(), unscaled)
    rec = a.validate(0)
    # a key-off trainer's metric path, fed the un-scaled raw prediction against the untouched data
    c = INRTrainer(_cfg(), image, coords, shape, dev, seed=3)
    want = c._device_metrics(c.image_full, unscaled.to(dev), False)[:2].cpu().tolist()
    print("psnr %.6f ssim %.6f test_loss %.6g" % (rec["psnr"], rec["ssim"], rec["test_loss"]))
    assert [rec["psnr"], rec["ssim"]] == want
    assert rec["test_loss"] == b.validate(0)["test_loss"]  # normalised units: the key-off fit's on the pre-scaled data
    assert rec["ring_normalization"] == a.ring_table.summary() and "ring_normalization" not in b.val_history[-1]
    m = a.metrics()
    assert [m["psnr"], m["ssim"]] == want and m["ring_normalization"]["rings"] == 3
    from inr_mi355x.evalchain import psnr, reconstruct
    assert a.evaluate() == float(psnr(reconstruct(c.image_full, shape, False), reconstruct(unscaled.to(dev), shape, False)))


def test_max_table_drives_a_fit(scan, dev):
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    tr = INRTrainer(_cfg(ring_normalization="max", partition=dict(no_steps=10, no_models=3), shuffle=True), image, coords,
                    shape, dev, seed=3)
    losses = _losses(tr, 5)
    assert len(losses) == 5 and all(np.isfinite(losses))
    t = tr.ring_table
    assert (t.stat, t.rings, t.no_steps, t.no_models) == ("max", 3, 10, 3) and t.radii[0] == 0.0 and t.radii[-1] == 5.0
    # the divisor of a ring is the largest |component| over its CLOSED interval, the scaling takes the half-open one:
    # the data divided by the divisor peak at 1 over the closed ring, and no normalised target of the ring exceeds 1
    d = torch.from_numpy(_radius(coords))
    for r in range(3):
        lo, hi = float(np.float32(t.radii[r])), float(np.float32(t.radii[r + 1]))
        closed = (d >= lo) & (d <= hi)
        assert float((image[closed].abs() / float(t.divisors[r])).max()) == 1.0
        assert float(tr.train_values.cpu()[(d >= lo) & (d < hi)].abs().max()) <= 1.0
    rec = tr.metrics()["ring_normalization"]
    assert rec == t.summary() and rec["stat"] == "max" and len(rec["radii"]) == 4 and len(rec["divisors"]) == 3
    ckpt = tr.checkpoint()
    assert set(ckpt) == {"net", "enc", "opt", "ring_normalization"}
    assert R.same_table(ckpt["ring_normalization"], t.state()) is None


def test_offgrid_fit_equals_key_off_fit_on_prescaled_samples(scan, table_file, dev):
    from inr_mi355x import trajectory as T
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    C, H, W = shape
    rows = T.trajectory_coords(T.spokes(H, W, 4), C, H, W)
    dist = _radius(rows)
    _assert_clear_of_the_table(dist)
    _assert_clear_of_the_table(_radius(coords))
    a = INRTrainer(_cfg(ring_normalization=table_file, trajectory="spokes-4", batch_size=40), image, coords, shape, dev,
                   seed=3)
    b = INRTrainer(_cfg(trajectory="spokes-4", batch_size=40), image, coords, shape, dev, seed=3)
    assert torch.equal(a.train_coords.cpu(), rows) and a.n_train == rows.shape[0] and a.n_train % 40 != 0
    # the key-off fit trains on ITS samples, pre-scaled on the host with the radius of their own coordinates
    pre = torch.from_numpy(R.ring_scale_numpy(dist, b.train_values.cpu(), **TABLE))
    assert _bits_equal(a.train_values.cpu(), pre)
    b.train_values.copy_(pre.to(dev))
    la, lb = _losses(a, 6), _losses(b, 6)
    assert len(la) == 6 and la == lb, (la, lb)
    assert _bits_equal(a.engine.params, b.engine.params)
    # the validation's targets: the full grid, normalised by one more call; the resident data stay what they were
    assert _bits_equal(a._norm_full.cpu(), torch.from_numpy(R.ring_scale_numpy(_radius(coords), image, **TABLE)))
    assert _bits_equal(a.image_full.cpu(), image)
    rec = a.validate(0)
    assert np.isfinite(rec["test_loss"]) and rec["ring_normalization"]["rings"] == 3 and rec["trajectory"]["spokes"] == 4


# ---- checkpoint and reconstruct ----------------------------------------------------------------------------------------
def test_reconstruct_from_a_normalised_checkpoint(scan, table_file, dev, tmp_path):
    from inr_mi355x.grid import GridSpec, grid_coords, grid_rows_numpy
    from inr_mi355x.reconstruct import Reconstructor
    from inr_mi355x.train import INRTrainer
    image, _, shape = scan
    C, H, W = shape
    _assert_clear_of_the_table(grid_rows_numpy(GridSpec(C, H, W), 0, C * H * W)[1])
    cfg = _cfg(ring_normalization=table_file)
    tr = INRTrainer(cfg, image, grid_coords(C, H, W, device=dev), shape, dev, seed=3)
    tr.fit(2)
    path = str(tmp_path / "model.pt")
    torch.save(tr.checkpoint(), path)
    rec = Reconstructor(cfg, path, shape=shape, device=dev)
    assert R.same_table(rec.ring_table.state(), tr.ring_table.state()) is None
    want = tr.predict_all(chunk=300)
    got = rec.render(chunk=300)
    assert got.shape == (C, H, W, 2) and _bits_equal(got.reshape(-1, 2), want)  # the native grid's tolerance: none
    # ... in the data's units: the raw sweep is a different tensor, and --compare's numbers are validate()'s
    assert not torch.equal(want, tr._predict_raw(chunk=300))
    v = tr.validate(0)
    cmp_ = rec.compare(got, image)
    assert abs(cmp_["psnr"] - v["psnr"]) <= 1e-9 * abs(v["psnr"]) and abs(cmp_["ssim"] - v["ssim"]) <= 1e-9
    # a checkpoint without the key renders as before, and does not load into a normalised trainer (nor the reverse)
    plain = INRTrainer(_cfg(), image, grid_coords(C, H, W, device=dev), shape, dev, seed=3)
    plain.fit(2)
    ck = plain.checkpoint()
    assert "ring_normalization" not in ck
    r2 = Reconstructor(_cfg(), ck, shape=shape, device=dev)
    assert r2.ring_table is None and _bits_equal(r2.render(chunk=300).reshape(-1, 2), plain.predict_all(chunk=300))
    with pytest.raises(ValueError, match="ring normalisation"):
        tr.load_checkpoint(ck)
    with pytest.raises(ValueError, match="ring normalisation"):
        plain.load_checkpoint(tr.checkpoint())
    other = dict(tr.checkpoint())
    other["ring_normalization"] = R.RingTable(TABLE["radii"], TABLE["divisors"] * np.float32(2), "file").state()
    with pytest.raises(ValueError, match="divisors"):
        tr.load_checkpoint(other)
    tr.load_checkpoint(tr.checkpoint())  # its own goes through


# ---- the search --------------------------------------------------------------------------------------------------------
def test_search_trial_leaves_the_cached_tensors_alone(table_file, dev):
    from inr_mi355x import hp_search as HS
    base = _cfg(max_epoch=1, normalization="coil", transform=False, log_iter=1000)
    runner = HS.LocalRunner(HS.synthetic_source(*SHAPE), 1, seed=0, device=dev, extra_key=SHAPE)
    image, coords, shape = runner.cache.get(base)
    keep = image.clone(), coords.clone()
    res = runner(dict(base, config_index=1, ring_normalization=table_file))
    assert "error" not in res, res
    assert res["ring_normalization"]["stat"] == "file" and res["ring_normalization"]["rings"] == 3
    assert res["best_psnr"] > 0 and res["steps"] == 4
    assert runner.cache.get(base)[0] is image and runner.cache.ingests == 1
    assert _bits_equal(image, keep[0]) and _bits_equal(coords, keep[1])
    plain = runner(dict(base, config_index=2))
    assert "ring_normalization" not in plain and "error" not in plain
    refused = runner(dict(base, config_index=3, ring_normalization="max", transform=True))
    assert "ring_normalization" in refused["error"]
