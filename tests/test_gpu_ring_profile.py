"""The continuous ring divisor on the MI355X (``-m gpu``): inr_radial_scale against
ringnorm.radial_scale_numpy bit for bit (whole groups and the partial last one, 16-byte and scalar access, in place and
out of place, one tile and several, nothing written past row n), its refusals, graph capture, and the trainer, the
checkpoint and ``reconstruct`` on top of it.

The trainer cases use an explicit table file, so they do not depend on k-means.  The host and the device may differ in the
last bit of a row's radius; the profile is continuous, so -- unlike under a step table -- that moves a target by a few
units in its last place and not by a ring's ratio.  Bit-equalities between a normalised fit and a key-off fit therefore
pre-scale with the radii the device computed, which is what the trainer scales with."""
import ctypes

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import ringnorm as R
from inr_mi355x.synthetic import make_kspace

pytestmark = pytest.mark.gpu

SENTINEL = 777.25
TAIL = 8  # sentinel rows behind row n - 1
SHAPE = (8, 16, 12)
TABLE = dict(radii=np.array([0.0, 0.3137, 0.7741, 5.0]), divisors=np.array([6.5, 0.75, 0.0625 * 1.3], dtype=np.float32))
KNOTS = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel --------------------------------------------------------------------------------------------------------
def _profile(n_knots: int, exact: bool):
    """(profile fp32, r_lo, inv_step): knots on exactly representable radii (``exact``: r_lo = 1/8, a power-of-two step
    that puts the last knot at or below 1.125) or on radii where s and u round"""
    rng = np.random.default_rng(7 * n_knots + exact)
    p = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), n_knots)).astype(np.float32)
    if exact:
        return p, np.float32(0.125), np.float32(2.0 ** int(np.ceil(np.log2(n_knots - 1))))
    return p, np.float32(0.05), np.float32((n_knots - 1) / 1.15)


def _rows(n: int, p, r_lo, inv_step):
    """dist [n] and values [n,2]: rows on knots (the first, the last, inner ones), one fp32 step beside them, below r_lo,
    beyond the last knot, NaN and infinite radii -- the special rows first, so that the smallest n still meet some -- and
    random rows in between; field values from subnormal to huge, of both signs"""
    rng = np.random.default_rng(n)
    knots = (r_lo + np.arange(p.size, dtype=np.float32) / inv_step).astype(np.float32)
    inner = knots[np.unique(np.linspace(0, p.size - 1, 9).astype(int))]
    special = np.concatenate([[knots[0], np.nan, knots[-1], 0.0], inner, [1.3, 7.0, np.inf, -np.inf, -2.0],
                              np.nextafter(inner, np.float32(-1)), np.nextafter(inner, np.float32(9))]).astype(np.float32)
    dist = rng.uniform(0.0, 1.45, n).astype(np.float32)
    k = min(n, special.size)
    dist[:k] = special[:k]
    values = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 2))) * rng.choice([-1.0, 1.0], (n, 2))).astype(np.float32)
    odd = np.array([1e-42, -3e-39, 3.0e38, -1.0e37, 0.0, -0.0, 1.2e-38, 2.5e35], np.float32)  # subnormal, huge, zeros
    m = min(2 * n, 4 * odd.size)
    values.reshape(-1)[:m] = np.tile(odd, 4)[:m]
    if n > special.size:  # spread them over the tiles
        order = rng.permutation(n)
        dist, values = dist[order], values[order]
    return dist, values


@pytest.mark.parametrize("multiply", [0, 1])
@pytest.mark.parametrize("n_knots", [2, 3, 1024, 4096])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_kernel_equals_numpy_bit_for_bit(dev, n, n_knots, multiply):
    for exact in (True, False):
        _check_kernel(dev, n, n_knots, multiply, exact)


def test_kernel_grid_stride_beyond_2048_tiles(dev):
    """more tiles of 1024 rows than the kernel launches blocks (2048): every block takes a second tile, some a partial one"""
    _check_kernel(dev, 2048 * 1024 + 1029, 1024, 0, False, offsets=(0,))
    _check_kernel(dev, 2048 * 1024 + 1029, 1024, 1, True, offsets=(1,))


def _check_kernel(dev, n, n_knots, multiply, exact, offsets=(0, 1)):
    p, r_lo, inv_step = _profile(n_knots, exact)
    dist, values = _rows(n, p, r_lo, inv_step)
    with np.errstate(all="ignore"):
        want_np = R.radial_scale_numpy(dist, values, p, r_lo, inv_step, bool(multiply))
    want = torch.from_numpy(want_np)
    nan = np.isnan(dist)
    assert np.array_equal(want_np[nan].view(np.uint32), values[nan].view(np.uint32))
    if n >= 64:  # the inputs hold what they are meant to
        with np.errstate(all="ignore"):
            u = (dist - r_lo) * inv_step
        assert nan.any() and (dist < r_lo).any() and (u > n_knots - 1).any()
        if exact:  # rows on the first, the last and -- where there are any -- inner knots
            assert (u == 0).any() and (u == n_knots - 1).any()
            assert n_knots == 2 or ((u == np.floor(u)) & (u > 0) & (u < n_knots - 1)).any()
        tiny = np.abs(values[values != 0]).min()
        assert tiny < 1.1754944e-38 and np.abs(values).max() > 1e38
    p_dev = torch.from_numpy(p).to(dev)
    for off in offsets:  # 16-byte aligned buffers; views that start one row in (dist 4-byte, in / out 8-byte aligned)
        rows = off + n + TAIL
        d_buf = torch.full((rows,), float("nan"), device=dev)
        d_buf[off:off + n] = torch.from_numpy(dist).to(dev)
        d_buf[off + n:] = float(r_lo) + 0.3  # rows behind n would be scaled if they were touched
        v_buf = torch.full((rows, 2), SENTINEL, device=dev)
        v_buf[off:off + n] = torch.from_numpy(values).to(dev)
        keep = v_buf.clone()
        d, v = d_buf[off:off + n], v_buf[off:off + n]
        assert d.data_ptr() % 16 == 4 * off and v.data_ptr() % 16 == 8 * off
        # out of place
        o_buf = torch.full((rows, 2), SENTINEL, device=dev)
        got = R.radial_scale(d, v, p_dev, r_lo, inv_step, bool(multiply), out=o_buf[off:off + n])
        assert got.data_ptr() == o_buf[off:off + n].data_ptr()
        assert _bits_equal(got.cpu(), want), (n, n_knots, multiply, exact, off)
        assert _bits_equal(v_buf, keep)  # `in` is unchanged
        assert bool((o_buf[:off] == SENTINEL).all()) and bool((o_buf[off + n:] == SENTINEL).all())
        # two calls give the same bits
        assert _bits_equal(R.radial_scale(d, v, p_dev, r_lo, inv_step, bool(multiply)), got)
        # in place
        assert R.radial_scale(d, v, p_dev, r_lo, inv_step, bool(multiply), out=v).data_ptr() == v.data_ptr()
        assert _bits_equal(v.cpu(), want), (n, n_knots, multiply, exact, off, "in place")
        assert bool((v_buf[:off] == SENTINEL).all()) and bool((v_buf[off + n:] == SENTINEL).all())
        # and back: the inverse operation on the same profile
        back = R.radial_scale(d, v, p_dev, r_lo, inv_step, not multiply).cpu()
        with np.errstate(all="ignore"):
            assert _bits_equal(back, torch.from_numpy(R.radial_scale_numpy(dist, want_np, p, r_lo, inv_step, not multiply)))
        # ... within two roundings of the input where neither step left the normal range
        a, b, w = back.double().abs(), torch.from_numpy(values).double().abs(), want.double().abs()
        normal = (b > 1e-30) & (b < 1e30) & (w > 1e-30) & (w < 1e30)
        if bool(normal.any()):
            assert float(((a - b).abs() / b)[normal].max()) <= 2.0 ** -22


def test_refusals_launch_nothing(dev):
    lib = L.load()
    n, knots = 64, 16
    dist = torch.rand(n, device=dev)
    vin = torch.ones(n + 2, 2, device=dev)
    out = torch.full((n + 2, 2), SENTINEL, device=dev)
    prof = torch.full((2 * n,), 2.0, device=dev)
    good = dict(dist=dist.data_ptr(), vin=vin.data_ptr(), out=out.data_ptr(), n=n, prof=prof.data_ptr(), knots=knots,
                r_lo=0.0, inv_step=15.0, multiply=0)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.inr_radial_scale(a["dist"], a["vin"], a["out"], a["n"], a["prof"], a["knots"], a["r_lo"], a["inv_step"],
                                  a["multiply"], torch.cuda.current_stream(dev).cuda_stream)
        return rc, L.last_error()

    nan, inf = float("nan"), float("inf")
    bad = [(dict(dist=None), "null"), (dict(vin=None), "null"), (dict(out=None), "null"), (dict(prof=None), "null"),
           (dict(n=0), "n = 0"), (dict(n=-5), "n = -5"), (dict(n=1 << 31), "n = 2147483648"),
           (dict(knots=1), "n_knots = 1"), (dict(knots=0), "n_knots"), (dict(knots=-4), "n_knots"),
           (dict(knots=4097), "n_knots = 4097"),
           (dict(r_lo=nan), "r_lo"), (dict(r_lo=inf), "r_lo"), (dict(r_lo=-inf), "r_lo"),
           (dict(inv_step=nan), "inv_step"), (dict(inv_step=inf), "inv_step"), (dict(inv_step=0.0), "inv_step"),
           (dict(inv_step=-15.0), "inv_step"),
           (dict(vin=vin.data_ptr() + 4), "aligned"), (dict(out=out.data_ptr() + 4), "aligned"),
           (dict(dist=dist.data_ptr() + 2), "aligned"), (dict(prof=prof.data_ptr() + 2), "profile must be 4-byte aligned"),
           (dict(vin=out.data_ptr() + 8), "overlaps in"), (dict(vin=out.data_ptr() + 8 * n - 8), "overlaps in"),
           (dict(vin=out.data_ptr() - 8 * n + 8), "overlaps in"),
           (dict(dist=out.data_ptr()), "overlaps dist"), (dict(dist=out.data_ptr() + 8 * n - 4), "overlaps dist"),
           (dict(prof=out.data_ptr()), "overlaps profile"), (dict(prof=out.data_ptr() + 8 * n - 4), "overlaps profile"),
           (dict(prof=out.data_ptr() - 4 * knots + 4), "overlaps profile")]
    for kw, text in bad:
        for multiply in (0, 1):
            rc, msg = call(multiply=multiply, **kw)
            assert rc == -1 and text in msg and msg.startswith("inr_radial_scale"), (kw, rc, msg)
    torch.cuda.synchronize(dev)
    assert bool((out == SENTINEL).all()), "a refused call launched"
    # the same arguments, unspoiled, go through: in place and multiplying included
    assert call()[0] == 0 and call(vin=out.data_ptr())[0] == 0 and call(multiply=1)[0] == 0
    torch.cuda.synchronize(dev)
    assert bool((out[n:] == SENTINEL).all()) and not bool((out[:n] == SENTINEL).any())


def test_capturable_in_a_graph(dev):
    p, r_lo, inv_step = _profile(1024, False)
    dist, values = _rows(1025, p, r_lo, inv_step)
    d, v, p_dev = torch.from_numpy(dist).to(dev), torch.from_numpy(values).to(dev), torch.from_numpy(p).to(dev)
    out = torch.zeros_like(v)
    R.radial_scale(d, v, p_dev, r_lo, inv_step, out=out)  # loads the library before the capture
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        R.radial_scale(d, v, p_dev, r_lo, inv_step, out=out)
    g.replay()
    torch.cuda.synchronize(dev)
    with np.errstate(all="ignore"):
        assert _bits_equal(out.cpu(), torch.from_numpy(R.radial_scale_numpy(dist, values, p, r_lo, inv_step)))


# ---- the trainer -------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=100, max_epoch=4, weight_decay=0.0, beta1=0.9, beta2=0.999,
               val_epoch=1, encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


def _smooth(**kw):
    return dict(ring_profile="geometric", ring_profile_knots=KNOTS, **kw)


@pytest.fixture(scope="module")
def scan():
    return make_kspace(*SHAPE)


@pytest.fixture(scope="module")
def table_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ring_profile") / "table.npz")
    np.savez(path, **TABLE)
    return path


@pytest.fixture(scope="module")
def curve():
    return R.ring_profile(TABLE["radii"], TABLE["divisors"], "geometric", KNOTS)


def _losses(tr, steps):
    return [v for _, v in tr.fit(steps, log_every=1)]


@pytest.fixture(scope="module")
def grid_pair(scan, table_file, curve, dev):
    """(normalised trainer, key-off trainer on data pre-scaled by radial_scale_numpy, their losses) after six steps"""
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    a = INRTrainer(_cfg(ring_normalization=table_file, **_smooth()), image, coords, shape, dev, seed=3)
    pre = torch.from_numpy(R.radial_scale_numpy(a._grid_dist.cpu(), image, *curve))
    b = INRTrainer(_cfg(), pre, coords, shape, dev, seed=3)
    return a, b, _losses(a, 6), _losses(b, 6)


def test_fit_equals_key_off_fit_on_prescaled_data(scan, grid_pair, curve, dev):
    a, b, la, lb = grid_pair
    image, coords, _ = scan
    assert len(la) == 6 and la == lb, (la, lb)
    assert _bits_equal(a.engine.params, b.engine.params)
    # the trainer scaled into a buffer of its own: the resident data and the caller's tensor are what they were
    assert _bits_equal(a.image_full.cpu(), image) and a.train_values.data_ptr() != a.image_full.data_ptr()
    assert a.image is a.image_full and _bits_equal(a.train_values, b.image_full)
    t = a.ring_table
    assert (t.stat, t.rings, t.profile, t.knots) == ("file", 3, "geometric", KNOTS) and b.ring_table is None
    assert t.normalized_max == float(a.train_values.abs().max())
    # the targets are not the step table's: rows away from the ring centres are divided by something else
    c = coords.cpu()
    host_dist = torch.sqrt(c[:, 1] ** 2 + c[:, 2] ** 2).numpy()
    step = torch.from_numpy(R.ring_scale_numpy(host_dist, image, **TABLE))
    assert not torch.equal(a.train_values.cpu(), step)
    # and the host's radii give the same targets within the continuity of the profile (no row changes ring)
    host = torch.from_numpy(R.radial_scale_numpy(host_dist, image, *curve))
    rel = ((a.train_values.cpu().double() - host.double()).abs() / host.double().abs().clamp_min(1e-30)).max()
    assert float(rel) <= 2.0 ** -23 * (1 + 5.0 * float(curve[2])), float(rel)  # neighbouring knots differ by < 5 x


def test_validation_scores_in_data_units(scan, grid_pair, curve, dev):
    from inr_mi355x.train import INRTrainer
    a, b, _, _ = grid_pair
    image, coords, shape = scan
    raw = a._predict_raw()
    assert _bits_equal(raw, b.predict_all())
    unscaled = torch.from_numpy(R.radial_scale_numpy(a._grid_dist.cpu(), raw.cpu(), *curve, multiply=True))
    assert _bits_equal(a.predict_all().cpu(), unscaled)
    rec = a.validate(0)
    # a key-off trainer's metric path, fed the un-scaled raw prediction against the untouched data
    c = INRTrainer(_cfg(), image, coords, shape, dev, seed=3)
    want = c._device_metrics(c.image_full, unscaled.to(dev), False)[:2].cpu().tolist()
    print("psnr %.6f ssim %.6f test_loss %.6g" % (rec["psnr"], rec["ssim"], rec["test_loss"]))
    assert [rec["psnr"], rec["ssim"]] == want
    assert rec["test_loss"] == b.validate(0)["test_loss"]  # normalised units: the key-off fit's on the pre-scaled data
    s = rec["ring_normalization"]
    assert s == a.ring_table.summary() and "ring_normalization" not in b.val_history[-1]
    assert (s["profile"], s["knots"]) == ("geometric", KNOTS) and s["normalized_max"] == a.ring_table.normalized_max
    m = a.metrics()
    assert [m["psnr"], m["ssim"]] == want and m["ring_normalization"]["profile"] == "geometric"


def test_reconstruct_from_a_smooth_checkpoint(scan, table_file, dev, tmp_path):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.reconstruct import Reconstructor
    from inr_mi355x.train import INRTrainer
    image, _, shape = scan
    C, H, W = shape
    cfg = _cfg(ring_normalization=table_file, **_smooth())
    tr = INRTrainer(cfg, image, grid_coords(C, H, W, device=dev), shape, dev, seed=3)
    tr.fit(2)
    ckpt = tr.checkpoint()
    assert ckpt["ring_normalization"]["profile"] == "geometric" and ckpt["ring_normalization"]["knots"] == KNOTS
    path = str(tmp_path / "model.pt")
    torch.save(ckpt, path)
    rec = Reconstructor(cfg, path, shape=shape, device=dev)
    assert rec.ring_table.smooth and R.same_table(rec.ring_table.state(), tr.ring_table.state()) is None
    want = tr.predict_all(chunk=300)
    got = rec.render(chunk=300)
    assert got.shape == (C, H, W, 2) and _bits_equal(got.reshape(-1, 2), want)  # the native grid's tolerance: none
    # ... un-scaled with the profile: the raw sweep times the profile, not times a ring's constant
    raw = tr._predict_raw(chunk=300)
    assert not torch.equal(want, raw)
    assert _bits_equal(want.cpu(), torch.from_numpy(R.radial_scale_numpy(tr._grid_dist.cpu(), raw.cpu(),
                                                                         *tr.ring_table.curve, multiply=True)))
    step = R.RingTable(TABLE["radii"], TABLE["divisors"], "file")
    assert not torch.equal(want, step.unscale(tr._grid_dist, raw.clone()))


def test_resume_under_another_profile_is_refused(scan, table_file, dev):
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    smooth = INRTrainer(_cfg(ring_normalization=table_file, **_smooth()), image, coords, shape, dev, seed=3)
    step = INRTrainer(_cfg(ring_normalization=table_file), image, coords, shape, dev, seed=3)
    linear = INRTrainer(_cfg(ring_normalization=table_file, ring_profile="linear", ring_profile_knots=KNOTS), image, coords,
                        shape, dev, seed=3)
    coarse = INRTrainer(_cfg(ring_normalization=table_file, ring_profile="geometric", ring_profile_knots=64), image,
                        coords, shape, dev, seed=3)
    with pytest.raises(ValueError, match="profile 'geometric' against 'step'"):
        step.load_checkpoint(smooth.checkpoint())
    with pytest.raises(ValueError, match="profile 'step' against 'geometric'"):
        smooth.load_checkpoint(step.checkpoint())
    with pytest.raises(ValueError, match="profile 'linear' against 'geometric'"):
        smooth.load_checkpoint(linear.checkpoint())
    with pytest.raises(ValueError, match="64 profile knots against 256"):
        smooth.load_checkpoint(coarse.checkpoint())
    smooth.load_checkpoint(smooth.checkpoint())  # its own goes through
    with pytest.raises(ValueError, match="without ring_normalization"):
        INRTrainer(_cfg(ring_profile="geometric"), image, coords, shape, dev, seed=3)


def test_step_profile_named_explicitly_changes_nothing(scan, table_file, dev):
    """the prescaled-equality construction of the step table with ring_profile: step written out"""
    from inr_mi355x.train import INRTrainer
    image, coords, shape = scan
    c = coords.cpu()
    dist = torch.sqrt(c[:, 1] ** 2 + c[:, 2] ** 2).numpy()
    gap = np.abs(dist.astype(np.float64)[:, None] - TABLE["radii"][None, 1:]).min()
    assert gap > 1e-5, gap  # no row within a rounding of a ring edge: the device puts every row in the host's ring
    pre = torch.from_numpy(R.ring_scale_numpy(dist, image, **TABLE))
    a = INRTrainer(_cfg(ring_normalization=table_file, ring_profile="step", ring_profile_knots=64), image, coords, shape,
                   dev, seed=3)
    b = INRTrainer(_cfg(), pre, coords, shape, dev, seed=3)
    k = INRTrainer(_cfg(ring_normalization=table_file), image, coords, shape, dev, seed=3)
    la, lb, lk = _losses(a, 6), _losses(b, 6), _losses(k, 6)
    assert len(la) == 6 and la == lb == lk, (la, lb, lk)
    assert _bits_equal(a.engine.params, b.engine.params) and _bits_equal(a.engine.params, k.engine.params)
    assert not a.ring_table.smooth and a.ring_table.summary() == k.ring_table.summary()
    assert set(a.checkpoint()["ring_normalization"]) == {"radii", "divisors", "stat", "no_steps", "no_models"}
