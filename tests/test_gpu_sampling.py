"""Weighted epochs on the MI355X (``-m gpu``): inr_row_cdf and inr_sample_epoch against the numpy restatement of
DESIGN.md section 4.23 -- exact: integers and copies -- and fits that train from weighted epoch buffers.

Sizes: the scan tile is 1024 rows (L.ROW_CDF_TILE) and the pass over the tile sums takes 1024 of them per round, so
1024 * 1024 + 1024 + 5 rows is the first shape whose tile sums need a second round."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 1024
N_LIST = [1, 63, 64, 65, TILE, TILE + 1, 3 * TILE + 3, TILE * TILE + TILE + 5]
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=64)
ENC = dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _weights(n, kind, seed=0):
    """(w fp32 [n], mask uint8 [n] or None): random weights with the feature ``kind``"""
    rng = np.random.default_rng(1000 * seed + n % 9973)
    w = (rng.random(n) + 0.01).astype(np.float32)
    mask = None
    if kind == "leading_zeros":
        w[:max(1, n // 3)] = 0.0
    elif kind == "trailing_zeros":
        w[n - max(1, n // 3):] = 0.0
    elif kind == "interior_zeros":  # longer than a tile where n allows it
        lo = n // 4
        w[lo:lo + max(1, min(n - lo - 1, TILE + 77))] = 0.0
    elif kind == "dominant":
        w[n // 2] = 1.0e6
    elif kind == "mask":
        mask = (rng.random(n) < 0.6).astype(np.uint8) * 3  # any non-zero byte keeps the row
    if n > 4:  # the tick rules, wherever they fall
        w[1], w[2], w[3] = np.nan, -1.0, -0.0
    if not ((w > 0) & (True if mask is None else mask != 0)).any():
        w[n - 1] = 1.0
        if mask is not None:
            mask[n - 1] = 1
    return w, mask


def _scale(w, mask):
    from inr_mi355x.sampling import default_scale
    ok = np.isfinite(w) & (w > 0) & (True if mask is None else mask != 0)
    return default_scale(float(w[ok].max()))


def _as_u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


# ---- the kernels against numpy, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["leading_zeros", "trailing_zeros", "interior_zeros", "dominant", "mask"])
@pytest.mark.parametrize("n", N_LIST)
def test_cdf_and_draw_equal_numpy(dev, n, kind):
    from inr_mi355x.sampling import device_draw, epoch_draw_numpy, row_cdf, row_cdf_numpy
    w, mask = _weights(n, kind)
    scale = _scale(w, mask)
    want = row_cdf_numpy(w, scale, mask)
    rc = row_cdf(torch.from_numpy(w).to(dev), None if mask is None else torch.from_numpy(mask).to(dev), rows=1)
    assert rc.scale == scale  # the default scale: the largest weight that can be drawn
    got = _as_u64(rc.cdf)
    assert got.dtype == want.dtype == np.uint64 and np.array_equal(got, want)
    assert rc.total_ticks == int(want[-1])
    assert rc.zero_weight_rows == int(np.count_nonzero(np.diff(want, prepend=np.uint64(0)) == 0))
    for m in sorted({n, max(1, n // 3), 2 * n + 5, 1}):
        order = device_draw(rc.cdf, m, 5, 2).cpu().numpy()
        assert order.dtype == np.int64 and np.array_equal(order, epoch_draw_numpy(want, m, 5, 2)), (n, kind, m)


def test_explicit_scale_and_unaligned_weights(dev):
    """a weight vector that starts one float into its allocation takes the scalar loads: the same integers"""
    from inr_mi355x.sampling import row_cdf, row_cdf_numpy
    n = 3 * TILE + 3
    w, mask = _weights(n, "mask", seed=3)
    store, mstore = torch.zeros(n + 1, device=dev), torch.zeros(n + 1, dtype=torch.uint8, device=dev)
    store[1:] = torch.from_numpy(w).to(dev)
    mstore[1:] = torch.from_numpy(mask).to(dev)
    assert store[1:].data_ptr() % 16 == 4 and mstore[1:].data_ptr() % 4 == 1
    for scale in (1000.0, 0.5 * _scale(w, mask)):
        want = row_cdf_numpy(w, scale, mask)
        aligned = row_cdf(store[1:].clone(), mstore[1:].clone(), scale=scale, rows=1)
        shifted = row_cdf(store[1:], mstore[1:], scale=scale, rows=1)
        assert np.array_equal(_as_u64(aligned.cdf), want) and np.array_equal(_as_u64(shifted.cdf), want)


def test_equal_weights_full_draw_is_the_device_order(dev):
    from inr_mi355x.sampling import device_draw, row_cdf
    from inr_mi355x.shuffle import device_order
    for n in (65, 3 * TILE + 3):
        rc = row_cdf(torch.full((n,), 0.37, device=dev))
        for seed, epoch in ((0, 0), (2 ** 40 + 3, 12)):
            assert torch.equal(device_draw(rc.cdf, n, seed, epoch), device_order(n, seed, epoch, dev))


# bs = 64 / 128: batch ends at wave edges; 100 / 777: inside a wave; 5000: larger than some m (one short batch)
@pytest.mark.parametrize("bs", [64, 100, 128, 777, 5000])
@pytest.mark.parametrize("with_mask", [False, True])
def test_gather_and_batch_counts(dev, bs, with_mask):
    from inr_mi355x.sampling import epoch_draw_numpy, row_cdf, sample_epoch
    n = 3 * TILE + 3
    g = torch.Generator().manual_seed(n + bs)
    coords, gt, dist = torch.rand(n, 3, generator=g), torch.randn(n, 2, generator=g), torch.rand(n, generator=g)
    w = torch.rand(n, generator=g) ** 3
    mask = (torch.rand(n, generator=g) < 0.37).to(torch.uint8) if with_mask else None
    d = dict(coords=coords.to(dev), gt=gt.to(dev), dist=dist.to(dev), mask=None if mask is None else mask.to(dev))
    # the CDF ignores the mask here, so that drawn rows carry both mask values and the counts have something to count
    rc = row_cdf(w.to(dev), rows=1)
    cdf = _as_u64(rc.cdf)
    for m in (n, n // 3, 2 * n + 5, 1):
        nb = -(-m // bs)
        out = dict(coords_out=torch.full((m, 3), -7.0, device=dev), gt_out=torch.full((m, 2), -7.0, device=dev),
                   dist_out=torch.full((m,), -7.0, device=dev),
                   mask_out=torch.full((m,), 9, dtype=torch.uint8, device=dev) if with_mask else None)
        counts = torch.full((nb,), -5, dtype=torch.int32, device=dev)
        order_out = torch.empty(m, dtype=torch.int64, device=dev)
        sample_epoch(rc.cdf, m, 11, 3, **d, **out, batch_size=bs, batch_counts=counts, order_out=order_out)
        order = torch.from_numpy(epoch_draw_numpy(cdf, m, 11, 3))
        assert torch.equal(order_out.cpu(), order)
        assert torch.equal(out["coords_out"].cpu(), coords[order])
        assert torch.equal(out["gt_out"].cpu(), gt[order])
        assert torch.equal(out["dist_out"].cpu(), dist[order])
        flags = torch.ones(m, dtype=torch.int64) if mask is None else mask[order].to(torch.int64)
        if mask is not None:
            assert torch.equal(out["mask_out"].cpu(), mask[order])
        want = [int(flags[b * bs:(b + 1) * bs].sum()) for b in range(nb)]
        assert counts.cpu().tolist() == want
        # a second call into the same buffers: the counts are zeroed by the call, not by the caller
        sample_epoch(rc.cdf, m, 11, 3, **d, **out, batch_size=bs, batch_counts=counts)
        assert counts.cpu().tolist() == want


# ---- argument errors: each refused before a launch --------------------------------------------------------------------
def _invalid(rc, match):
    from inr_mi355x import _lib as L
    assert rc == -1, rc
    assert match in L.last_error(), L.last_error()


def test_row_cdf_error_codes(dev):
    from inr_mi355x import _lib as L
    lib = L.load()
    n = 2000
    w = torch.ones(n, device=dev)
    cdf = torch.full((n,), -3, dtype=torch.int64, device=dev)
    scratch = torch.zeros(2, dtype=torch.int64, device=dev)
    words = C.c_int64(0)
    assert lib.inr_row_cdf_scratch(n, C.byref(words)) == 0 and words.value == 2
    assert lib.inr_row_cdf_scratch(TILE, C.byref(words)) == 0 and words.value == 1
    _invalid(lib.inr_row_cdf_scratch(0, C.byref(words)), "n = 0")
    _invalid(lib.inr_row_cdf_scratch(2 ** 31, C.byref(words)), "n = 2147483648")
    _invalid(lib.inr_row_cdf_scratch(n, None), "null")
    call = lambda *a: lib.inr_row_cdf(*a, None)
    ok = [w.data_ptr(), None, n, C.c_double(1.0), cdf.data_ptr(), scratch.data_ptr(), 2]

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a

    _invalid(call(*with_(0, None)), "null")
    _invalid(call(*with_(4, None)), "null")
    _invalid(call(*with_(5, None)), "null")
    _invalid(call(*with_(2, 0)), "n = 0")
    _invalid(call(*with_(2, 2 ** 31)), "n = 2147483648")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _invalid(call(*with_(3, C.c_double(bad))), "scale")
    _invalid(call(*with_(6, 1)), "scratch holds 1 words, needs 2")
    _invalid(call(*with_(0, w.data_ptr() + 2)), "aligned")
    _invalid(call(*with_(4, cdf.data_ptr() + 4)), "aligned")
    _invalid(call(*with_(5, cdf.data_ptr())), "overlaps")
    torch.cuda.synchronize()
    assert bool((cdf == -3).all())  # nothing was launched
    assert call(*ok) == 0
    assert cdf.cpu().tolist() == list(range(1, n + 1))


def test_sample_epoch_error_codes(dev):
    from inr_mi355x import _lib as L
    lib = L.load()
    n, m = 300, 200
    cdf = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
    c, co = torch.zeros(n, 3, device=dev), torch.full((m, 3), -7.0, device=dev)
    g, go = torch.zeros(n, 2, device=dev), torch.zeros(m, 2, device=dev)
    mk, mo = torch.ones(n, dtype=torch.uint8, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)

    def call(cdf_=cdf.data_ptr(), n_=n, m_=m, bs=100, coords=None, gt=None, dist=None, mask=None, coords_out=None,
             gt_out=None, dist_out=None, mask_out=None, counts=None, order=None):
        return lib.inr_sample_epoch(cdf_, n_, m_, bs, C.c_uint64(1), C.c_uint32(0), coords, gt, dist, mask, coords_out,
                                    gt_out, dist_out, mask_out, counts, order, None)

    P = lambda t: t.data_ptr()
    _invalid(call(cdf_=None, coords=P(c), coords_out=P(co)), "null")
    _invalid(call(cdf_=P(cdf) + 4, coords=P(c), coords_out=P(co)), "aligned")
    _invalid(call(n_=0, coords=P(c), coords_out=P(co)), "n = 0")
    _invalid(call(n_=2 ** 31, coords=P(c), coords_out=P(co)), "n = 2147483648")
    _invalid(call(m_=0, coords=P(c), coords_out=P(co)), "m = 0")
    _invalid(call(m_=2 ** 31, coords=P(c), coords_out=P(co)), "m = 2147483648")
    # the buffer rules of inr_shuffle_epoch, with its messages
    _invalid(call(coords=P(c)), "an input and its output buffer go together")
    _invalid(call(gt_out=P(go)), "an input and its output buffer go together")
    _invalid(call(dist=P(c)), "an input and its output buffer go together")
    _invalid(call(mask_out=P(mo)), "an input and its output buffer go together")
    _invalid(call(), "no output")
    _invalid(call(mask=P(mk)), "no output")
    _invalid(call(bs=0, counts=P(cnt)), "batch_counts with batch_size = 0")
    _invalid(call(bs=2 ** 31, counts=P(cnt)), "batch_counts with batch_size = 2147483648")
    _invalid(call(gt=P(g) + 4, gt_out=P(go)), "8-byte aligned")
    _invalid(call(coords=P(c), coords_out=P(c)), "in-place")
    torch.cuda.synchronize()
    assert bool((co == -7.0).all())  # nothing was launched
    assert call(coords=P(c), coords_out=P(co), mask=P(mk), counts=P(cnt)) == 0  # a mask may come without mask_out
    assert cnt.cpu().tolist() == [100, 100]


def test_stride_zero_through_the_raw_entry(dev):
    """T < m: defined -- every position takes the row of threshold 0 -- and refused by the Python layer"""
    from inr_mi355x import _lib as L
    from inr_mi355x.sampling import epoch_draw_numpy, row_cdf, row_cdf_numpy
    lib = L.load()
    n, m = 500, 400
    w = np.zeros(n, np.float32)
    w[[123, 321]] = 1.0e-3
    for scale, first in ((1000.0, 123), (10.0, 0)):  # T = 2, then T = 0 (the ticks round down to none)
        wd = torch.from_numpy(w).to(dev)
        cdf = torch.empty(n, dtype=torch.int64, device=dev)
        scratch = torch.empty(1, dtype=torch.int64, device=dev)
        assert lib.inr_row_cdf(wd.data_ptr(), None, n, C.c_double(scale), cdf.data_ptr(), scratch.data_ptr(), 1, None) == 0
        assert np.array_equal(_as_u64(cdf), row_cdf_numpy(w, scale))
        order = torch.full((m,), -1, dtype=torch.int64, device=dev)
        assert lib.inr_sample_epoch(cdf.data_ptr(), n, m, 0, C.c_uint64(3), C.c_uint32(1), None, None, None, None, None,
                                    None, None, None, None, order.data_ptr(), None) == 0
        got = order.cpu().numpy()
        assert got.min() >= 0 and got.max() < n and np.all(got == first)
        assert np.array_equal(got, epoch_draw_numpy(_as_u64(cdf), m, 3, 1))
        with pytest.raises(ValueError, match="ticks"):
            row_cdf(wd, scale=scale, rows=m)
    with pytest.raises(ValueError, match="positive"):
        row_cdf(torch.zeros(n, device=dev))
    with pytest.raises(ValueError, match="scale"):
        row_cdf(torch.ones(n, device=dev), scale=float("inf"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        row_cdf(torch.ones(n))


# ---- fits --------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=200, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               net=dict(NET), encoder=dict(ENC), shuffle_seed=9)
    cfg.update(kw)
    return cfg


@pytest.fixture(scope="module")
def scan():
    from inr_mi355x.synthetic import make_kspace
    return make_kspace(3, 24, 20)


def _fit(cfg, scan, dev, **kw):
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3, **kw)
    losses = [float(s[1]) for s in tr.fit(log_every=1)]
    return tr, losses


def test_uniform_sampling_is_bitwise_the_shuffled_fit(dev, scan):
    for loss in ("L2", "HDR"):
        a, la = _fit(_cfg(loss=loss, shuffle=True), scan, dev)
        b, lb = _fit(_cfg(loss=loss, row_sampling="uniform"), scan, dev)
        assert len(la) == len(lb) == 2 * a.steps_per_epoch == 16
        assert la == lb and torch.equal(a.engine.params, b.engine.params)
        assert set(b.checkpoint()) == {"net", "enc", "opt"}


def test_masked_fit_draws_sampled_rows_only(dev, scan):
    tr, losses = _fit(_cfg(row_sampling="uniform", undersampling="grid-3*2", max_epoch=1), scan, dev)
    n, bs = tr.n_train, 200
    assert tr.mask is not None and 0 < int(tr.mask.sum()) < n
    assert tr._epoch_buf.counts == [bs] * (n // bs) + ([n % bs] if n % bs else [])
    assert bool(tr._t_mask.all()) and bool(tr.mask[tr._epoch_buf.draw(0)].all())
    assert tr._epoch_buf.summary()["zero_weight_rows"] == n - int(tr.mask.sum())
    assert all(np.isfinite(losses))


def test_live_weights_take_effect_at_the_next_epoch(dev, scan):
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    tr = INRTrainer(_cfg(row_sampling="uniform", max_epoch=3), image, coords, shape, dev, seed=3)
    n = tr.n_train
    w = torch.ones(n, device=dev)
    dead = torch.arange(n, device=dev) % 2 == 1
    w[dead] = 0.0
    seen = []

    def on_epoch_end(epoch):
        seen.append(tr._epoch_buf.draw(epoch))
        if epoch == 0:
            tr.set_row_weights(w)

    tr.fit(on_epoch_end=on_epoch_end)
    assert torch.equal(torch.sort(seen[0])[0], torch.arange(n, device=dev))  # epoch 0: uniform, every row once
    order1 = tr._epoch_buf.draw(1)
    assert not bool(dead[order1].any()) and not bool(dead[tr._epoch_buf.draw(2)].any())
    # ... and the buffers of the epoch that followed held exactly that draw
    tr2 = INRTrainer(_cfg(row_sampling="uniform", max_epoch=3), image, coords, shape, dev, seed=3)
    tr2.set_row_weights(w)
    tr2._epoch_buf.begin(1)
    assert torch.equal(tr2._t_coords, tr.coords[order1])
    assert tr.metrics()["row_sampling"]["mode"] == "weights"
    with pytest.raises(ValueError):
        tr.set_row_weights(torch.ones(n - 1, device=dev))
    plain = INRTrainer(_cfg(), image, coords, shape, dev, seed=3)
    with pytest.raises(RuntimeError, match="row_sampling"):
        plain.set_row_weights(w)


def test_records_carry_row_sampling(dev, scan, tmp_path):
    image, coords, shape = scan
    path = str(tmp_path / "w.npy")
    wfile = np.linspace(0.0, 1.0, coords.shape[0]).astype(np.float32)
    np.save(path, wfile)
    for spec, mode in (("uniform", "uniform"), ("ring-inverse", "ring-inverse"), (path, path)):
        tr, _ = _fit(_cfg(row_sampling=spec, max_epoch=1, partition=dict(no_steps=10, no_models=3)), scan, dev)
        rec = tr.validate(0)
        info = rec["row_sampling"]
        assert set(info) == {"mode", "rows", "zero_weight_rows", "total_ticks"}
        assert info["mode"] == mode and info["rows"] == tr.n_train and info["total_ticks"] >= 2 ** 32 - 1
        assert info["zero_weight_rows"] == (1 if spec == path else 0)
        assert tr.metrics()["row_sampling"] == info
        if spec == "ring-inverse":  # the outermost ring's rows weigh 1, every ring inside it less: its maximum is larger
            w = np.diff(_as_u64(tr._epoch_buf.row_cdf.cdf), prepend=np.uint64(0)) / tr._epoch_buf.row_cdf.scale
            radius = torch.sqrt(tr.coords[:, 1] ** 2 + tr.coords[:, 2] ** 2).cpu().numpy()
            assert abs(w[radius.argmax()] - 1.0) < 1e-6 and w[radius.argmin()] < 1.0 and len(np.unique(w.round(6))) == 3
    plain, _ = _fit(_cfg(max_epoch=1), scan, dev)
    assert "row_sampling" not in plain.validate(0) and "row_sampling" not in plain.metrics()


def test_refusals(dev, scan):
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    make = lambda cfg, **kw: INRTrainer(cfg, image, coords, shape, dev, seed=3, **kw)
    with pytest.raises(ValueError, match="graph_steps"):
        make(_cfg(row_sampling="uniform"), graph_steps=True)
    with pytest.raises(ValueError, match="per_coil"):
        make(_cfg(row_sampling="uniform", per_coil=True))
    with pytest.raises(ValueError, match="use_tv"):
        make(_cfg(row_sampling="uniform", use_tv=True))
    with pytest.raises(NotImplementedError, match="LSL"):
        make(_cfg(row_sampling="uniform", loss="LSL"))
    with pytest.raises(NotImplementedError, match="rank"):
        make(_cfg(row_sampling="uniform"), rank=0, world=2)
    with pytest.raises(ValueError, match="trajectory"):
        make(_cfg(row_sampling="density"))
    with pytest.raises(ValueError, match="row_sampling"):
        make(_cfg(row_sampling="heavy"))
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    other = _cfg(row_sampling="uniform", model="Fourier", partition=dict(no_steps=10, no_models=2))
    with pytest.raises(NotImplementedError, match="INRTrainer"):
        MultiscaleTrainer(other, image, coords, None, None, shape, dev)
    with pytest.raises(NotImplementedError, match="INRTrainer"):
        RingEnsembleTrainer(other, image, coords, shape, dev)


def test_density_draw_follows_the_ramp(dev, scan):
    """spokes-8-24: the rows drawn per readout index, summed over spokes and coils, lie within the count bounds"""
    tr, losses = _fit(_cfg(row_sampling="density", trajectory="spokes-8-24", max_epoch=1, batch_size=144), scan, dev)
    C_, S_, R = 3, 8, 24
    n = tr.n_train
    assert n == C_ * S_ * R and all(np.isfinite(losses))
    buf = tr._epoch_buf
    cdf = _as_u64(buf.row_cdf.cdf)
    q = np.diff(cdf, prepend=np.uint64(0))
    stride = int(cdf[-1]) // n
    assert int(cdf[-1]) % n < stride
    got = np.bincount(buf.draw(0).cpu().numpy(), minlength=n)
    k = np.array([int(v) // stride for v in q])
    assert np.all(got >= np.maximum(0, k - 1)) and np.all(got <= k + 2)
    per_index = got.reshape(C_ * S_, R).sum(axis=0)
    lo, hi = np.maximum(0, k - 1).reshape(C_ * S_, R).sum(axis=0), (k + 2).reshape(C_ * S_, R).sum(axis=0)
    assert np.all(per_index >= lo) and np.all(per_index <= hi)
    j = np.abs(np.arange(R) - R // 2).astype(np.float64)
    j[R // 2] = 0.25
    # the ramp itself: the expected rows of readout index j are n * j / sum(j) per (coil, spoke) pair
    want = n * j / (j.sum() * C_ * S_)
    assert np.all(np.abs(got.reshape(C_ * S_, R) - want[None, :]) < 2.0)
    assert tr.validate(0)["row_sampling"]["mode"] == "density"
