"""Radial band statistics on the MI355X (``-m gpu``): inr_band_stats (csrc/inr_bands.hip) against its
numpy restatement bands.band_stats_numpy, the clustering functions on device tensors against the same functions on the
CPU copies, and the opt-in band report of the trainers and of Reconstructor.compare.

Tolerances: ``n``, every extremum and ``max_abs2`` are exact.  The two sums (``energy``, ``sse``) are sums of n
non-negative fp64 terms formed identically on both sides and added in different orders: each side is within n 2^-53
(relative, to first order) of the exact sum, so they agree within 2 n 2^-53 -- derived, not tuned.

Shapes: n around the wave (63, 64, 65), around one workgroup tile of 1024 rows (tile - 1, tile, tile + 1, 3 tiles + 7),
n = 1, and 65 543 rows = 17 workgroups of 4 tiles each with a ragged last tile (more than one partial per band, more than
one tile per workgroup); K in {1, 2, 40, 64}.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import bands as B

pytestmark = pytest.mark.gpu

TILE = L.BAND_TILE_ROWS
SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 7, 64 * TILE + 7]
SUM_FIELDS, EXACT_FIELDS = ("energy", "sse"), ("n", "max_abs2", "max_comp", "min_comp", "max_err2")
SHAPE = (2, 32, 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bounds(K):
    if K == 1:
        return [(0.2, 1.1)]
    if K == 2:
        return [(0.0, 0.75), (0.5, 5.0)]  # overlapping
    b = B.ring_bounds(40)
    if K == 64:  # rings, then nested / overlapping / empty / degenerate bands
        b = b + [(0.1 * i, 1.5 - 0.05 * i) for i in range(10)] + [(2.0, 3.0)] * 4 + [(0.5, 0.5)] * 10
    assert len(b) == K
    return b


_inputs_cache = {}


def _inputs(n, dev):
    """(host, device) copies of dist, gt, pred, mask for n rows: made once per n, never modified"""
    if n not in _inputs_cache:
        g = torch.Generator().manual_seed(1000 + n)
        dist = torch.rand(n, generator=g) * 1.45
        ring = B.ring_bounds(40)
        for k, row in enumerate(range(0, n, max(1, n // 23))):  # exact boundary hits: fp32 values of ring ends
            dist[row] = float(np.float32(ring[(5 * k) % 40][1]))
        gt = torch.randn(n, 2, generator=g) * torch.exp(-4 * dist).reshape(-1, 1)
        pred = gt + 0.03 * torch.randn(n, 2, generator=g)
        mask = (torch.rand(n, generator=g) < 0.4).to(torch.uint8) * 3
        host = (dist, gt, pred, mask)
        _inputs_cache[n] = (host, tuple(t.to(dev) for t in host))
    return _inputs_cache[n]


def _assert_equal(got, want, n_rows, what=""):
    tol = 2.0 * n_rows * 2.0 ** -53
    assert np.array_equal(got.lo, want.lo) and np.array_equal(got.hi, want.hi)
    for f in EXACT_FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f, getattr(got, f), getattr(want, f))
    for f in SUM_FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        rel = np.abs(a - b) / np.where(b == 0, 1.0, np.abs(b))
        print(f"{what} {f}: max rel diff {rel.max():.3g} (bound {tol:.3g})")
        assert np.all(np.abs(a - b) <= tol * np.abs(b)), (what, f, a, b)


@pytest.mark.parametrize("K", [1, 2, 40, 64])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_numpy(dev, n, K):
    (dist, gt, pred, _), (d_dist, d_gt, d_pred, _) = _inputs(n, dev)
    bounds = _bounds(K)
    got = B.band_stats(d_dist, d_gt, d_pred, bounds=bounds)
    _assert_equal(got, B.band_stats_numpy(dist, gt, pred, bounds=bounds), n, f"n={n} K={K}")
    if K == 64:
        assert np.all(got.n[50:54] == 0) and np.all(got.min_comp[50:54] == math.inf)  # the bands nothing lies in


@pytest.mark.parametrize("n", [65, TILE + 1, 64 * TILE + 7])
def test_masks_pred_null_and_unaligned(dev, n):
    (dist, gt, pred, mask), (d_dist, d_gt, d_pred, d_mask) = _inputs(n, dev)
    bounds = _bounds(40)
    whole = B.band_stats(d_dist, d_gt, d_pred, bounds=bounds)
    whole = B.BandStats(*(np.copy(a) for a in whole))
    halves = []
    for sel in (1, 0):
        got = B.band_stats(d_dist, d_gt, d_pred, mask=d_mask, mask_select=sel, bounds=bounds)
        _assert_equal(got, B.band_stats_numpy(dist, gt, pred, mask=mask, mask_select=sel, bounds=bounds), n, f"sel={sel}")
        halves.append(got)
    assert np.array_equal(halves[0].n + halves[1].n, whole.n)
    assert np.array_equal(np.maximum(halves[0].max_err2, halves[1].max_err2), whole.max_err2)
    none = B.band_stats(d_dist, d_gt, None, bounds=bounds)
    _assert_equal(none, B.band_stats_numpy(dist, gt, None, bounds=bounds), n, "pred=None")
    assert np.all(none.sse == 0) and np.all(none.max_err2 == -math.inf)
    if n > 8:  # views that start 4 / 8 / 1 bytes into their buffers: the 4-byte path
        got = B.band_stats(d_dist[1:], d_gt[1:], d_pred[1:], mask=d_mask[1:], bounds=bounds)
        _assert_equal(got, B.band_stats_numpy(dist[1:], gt[1:], pred[1:], mask=mask[1:], bounds=bounds), n, "unaligned")


def test_all_bands_empty(dev):
    _, (d_dist, d_gt, d_pred, _) = _inputs(3 * TILE + 7, dev)
    got = B.band_stats(d_dist, d_gt, d_pred, bounds=[(2.0, 3.0), (4.0, 4.0), (-2.0, -1.0)])
    assert np.all(got.n == 0) and np.all(got.energy == 0) and np.all(got.sse == 0)
    for f in ("max_abs2", "max_comp", "max_err2"):
        assert np.all(getattr(got, f) == -math.inf)
    assert np.all(got.min_comp == math.inf)


def test_boundary_rows_count_twice(dev):
    ring = B.ring_bounds(8)
    edges = torch.tensor([float(np.float32(ring[i][1])) for i in range(7)] * 3)
    gt = torch.ones(edges.numel(), 2)
    got = B.band_stats(edges.to(dev), gt.to(dev), bounds=ring)
    want = B.band_stats_numpy(edges, gt, bounds=ring)
    _assert_equal(got, want, edges.numel())
    assert int(got.n.sum()) == 2 * edges.numel() and got.n[0] == 3 and got.n[3] == 6


def _call(dist, gt, lo, hi, K, stats, scratch, n=None):
    FP = C.POINTER(C.c_float)
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    return L.load().inr_band_stats(dist.data_ptr(), gt.data_ptr(), None, None, 1, dist.numel() if n is None else n,
                                   lo.ctypes.data_as(FP), hi.ctypes.data_as(FP), K, stats.data_ptr(), scratch.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)


def test_refusals_launch_nothing(dev):
    _, (d_dist, d_gt, _, _) = _inputs(TILE + 1, dev)
    stats = torch.full((64, L.BAND_FIELDS), 123.0, device=dev, dtype=torch.float64)
    scratch = torch.full((B.scratch_doubles(TILE + 1, 64),), 321.0, device=dev, dtype=torch.float64)
    ones, zeros = [1.0] * 65, [0.0] * 65
    cases = {"K = 0": (zeros, ones, 0, None), "K = 65": (zeros, ones, 65, None), "lo > hi": ([0.0, 0.6], [1.0, 0.5], 2, None),
             "NaN bound": ([0.0, math.nan], [1.0, 1.0], 2, None), "n = 0": (zeros, ones, 1, 0),
             "n = 2^31": (zeros, ones, 1, 1 << 31)}
    for what, (lo, hi, K, n) in cases.items():
        assert _call(d_dist, d_gt, lo, hi, K, stats, scratch, n) == -1, what  # INR_ERR_INVALID
        assert L.last_error().startswith("inr_band_stats: "), (what, L.last_error())
    torch.cuda.synchronize()
    assert bool((stats == 123.0).all()) and bool((scratch == 321.0).all())  # nothing ran
    out = C.c_int64(-5)
    for n, K in ((TILE, 0), (TILE, 65), (0, 4), (1 << 31, 4)):
        assert L.load().inr_band_stats_scratch(n, K, C.byref(out)) == -1 and out.value == -5
    for bad in ([], [(0.0, 1.0)] * 65, [(0.6, 0.5)], [(math.nan, 1.0)]):  # the wrapper refuses them itself
        with pytest.raises(ValueError):
            B.band_stats(d_dist, d_gt, bounds=bad)
    with pytest.raises(RuntimeError):  # no CPU fallback
        B.band_stats(d_dist.cpu(), d_gt.cpu(), bounds=[(0.0, 1.0)])


def test_scratch_is_a_function_of_n_and_k():
    for n, blocks in ((1, 1), (4 * TILE, 1), (4 * TILE + 1, 2), (64 * TILE + 7, 17), (15 * 640 * 368, 863)):
        assert B.scratch_doubles(n, 40) == blocks * 40 * L.BAND_FIELDS
    assert B.scratch_doubles((1 << 31) - 1, 64) == 2048 * 64 * L.BAND_FIELDS


def test_two_calls_bit_identical(dev):
    n = 64 * TILE + 7
    _, (d_dist, d_gt, d_pred, d_mask) = _inputs(n, dev)
    bounds = _bounds(64)
    first = B.band_stats_device(d_dist, d_gt, d_pred, d_mask, 1, bounds)[2].clone()
    (torch.randn(1 << 16, device=dev) * 2).sum()  # an unrelated launch in between
    B.band_stats(d_dist, d_gt, None, bounds=_bounds(2))
    again = B.band_stats_device(d_dist, d_gt, d_pred, d_mask, 1, bounds)[2]
    assert torch.equal(first.view(torch.int64), again.view(torch.int64))


# ---- clustering on the kernel ------------------------------------------------------------------------------------------
def test_clustering_on_device_equals_cpu(dev):
    from inr_mi355x.clustering import partition_and_stats, partition_kspace
    from inr_mi355x.synthetic import make_kspace
    Cc, H, W = SHAPE
    image, coords, _ = make_kspace(Cc, H, W)
    img, kc = image.reshape(Cc, H, W, 2), coords.reshape(Cc, H, W, 3)
    labels, radii = partition_kspace(img, kc, no_steps=8, no_parts=3)
    d_labels, d_radii = partition_kspace(img.to(dev), kc.to(dev), no_steps=8, no_parts=3)
    assert np.array_equal(labels, d_labels) and np.array_equal(radii, d_radii)
    for stat in ("max", "min"):
        want, r = partition_and_stats(img, kc, 8, 3, stat=stat)
        got, d_r = partition_and_stats(img.to(dev), kc.to(dev), 8, 3, stat=stat)
        assert got.device.type == "cuda" and got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got.cpu(), want) and np.array_equal(r, d_r)
    with pytest.raises(RuntimeError, match="holds no k-space point"):  # an empty ring stays an error
        far = kc.clone()
        far[..., 1:] = far[..., 1:] * 0.5  # nothing beyond radius 0.71: the outer rings are empty
        partition_kspace(img.to(dev), far.to(dev), no_steps=8, no_parts=3)


def test_clustering_more_rings_than_one_call_and_other_dtypes(dev):
    """70 rings are two kernel calls (64 + 6); a float64 k-space keeps the loop of masked reductions.  Both equal the CPU
    result.  The points lie on a spiral whose radius grows evenly to sqrt(2), so that each of the 70 rings holds some."""
    from inr_mi355x.clustering import partition_and_stats, partition_kspace
    from inr_mi355x.synthetic import make_kspace
    Cc, H, W = SHAPE
    image, coords, _ = make_kspace(Cc, H, W)
    n = Cc * H * W
    r = math.sqrt(2) * (torch.arange(n, dtype=torch.float64) + 0.5) / n
    ang = torch.arange(n, dtype=torch.float64) * 0.61
    kc = coords.clone()
    kc[:, 1], kc[:, 2] = (r * torch.cos(ang)).float(), (r * torch.sin(ang)).float()
    img, kc = image.reshape(Cc, H, W, 2), kc.reshape(Cc, H, W, 3)
    for cast in (lambda t: t, lambda t: t.double()):
        labels, radii = partition_kspace(cast(img), cast(kc), no_steps=70, no_parts=3)
        d_labels, d_radii = partition_kspace(cast(img).to(dev), cast(kc).to(dev), no_steps=70, no_parts=3)
        assert len(labels) == 70 and np.array_equal(labels, d_labels) and np.array_equal(radii, d_radii)
        want, _ = partition_and_stats(cast(img), cast(kc), 70, 3)
        got, _ = partition_and_stats(cast(img).to(dev), cast(kc).to(dev), 70, 3)
        assert got.dtype == want.dtype and torch.equal(got.cpu(), want)


# ---- the opt-in report -------------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=500, max_epoch=3, weight_decay=0.0, beta1=0.9, beta2=0.999,
               val_epoch=1, partition=dict(no_steps=8, no_models=3),
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


def _assert_report(got, want, n_rows):
    """a record's report against band_report of the numpy statistics: sums within the bound above, the rest exact"""
    tol = 2.0 * n_rows * 2.0 ** -53
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in ("lo", "hi", "n", "max_abs_err"):
            assert g[k] == w[k], (k, g, w)
        for k in ("energy", "sse"):
            assert abs(g[k] - w[k]) <= tol * abs(w[k]), (k, g, w)
        if w["err_db"] is None:
            assert g["err_db"] is None
        else:  # d(10 log10 x) = 4.35 dx / x, for the quotient of two sums
            assert abs(g["err_db"] - w["err_db"]) <= 10.0 * tol, (g, w)


def _trainer_pair(dev, **kw):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(*SHAPE)
    out = []
    for report in (False, True):
        tr = INRTrainer(_cfg(**kw), image, coords, shape, dev, seed=3)
        if report:
            tr.enable_band_report()
        recs = []
        tr.fit(val_epoch=1, on_validate=recs.append)
        out.append((tr, recs))
    return image, coords, out


def test_trainer_report_changes_nothing_and_matches_numpy(dev):
    image, coords, ((plain, recs0), (tr, recs1)) = _trainer_pair(dev)
    assert torch.equal(plain.engine.params.view(torch.int32), tr.engine.params.view(torch.int32))
    assert len(recs0) == len(recs1) == 3
    for a, b in zip(recs0, recs1):
        assert "bands" not in a and not any(k.startswith("bands") for k in a)
        assert set(b) - set(a) == {"bands"} and all(a[k] == b[k] for k in a)
    assert "bands" not in plain.metrics()
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    want = B.band_report(B.band_stats_numpy(dist, image, tr.predict_all().cpu(), bounds=B.ring_bounds(8)))
    _assert_report(recs1[-1]["bands"], want, dist.numel())
    _assert_report(tr.metrics()["bands"], want, dist.numel())
    assert len(want) == 8 and all(r["err_db"] is not None for r in want)
    tr.enable_band_report([(0.0, 0.3), (0.2, 5.0)])
    want2 = B.band_report(B.band_stats_numpy(dist, image, tr.predict_all().cpu(), bounds=[(0.0, 0.3), (0.2, 5.0)]))
    _assert_report(tr.metrics()["bands"], want2, dist.numel())


def test_undersampled_trainer_reports_sampled_and_unsampled(dev):
    image, coords, ((plain, recs0), (tr, recs1)) = _trainer_pair(dev, undersampling="grid-2*2")
    assert torch.equal(plain.engine.params.view(torch.int32), tr.engine.params.view(torch.int32))
    assert all("bands" not in r and "bands_sampled" not in r for r in recs0)
    assert set(recs1[-1]) - set(recs0[-1]) == {"bands", "bands_sampled", "bands_unsampled"}
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    pred, mask = tr.predict_all().cpu(), tr.mask_cpu.reshape(-1)
    assert 0 < int((mask != 0).sum()) < mask.numel()
    for key, kw in (("bands", {}), ("bands_sampled", dict(mask=mask, mask_select=1)),
                    ("bands_unsampled", dict(mask=mask, mask_select=0))):
        want = B.band_report(B.band_stats_numpy(dist, image, pred, bounds=B.ring_bounds(8), **kw))
        _assert_report(recs1[-1][key], want, dist.numel())
    n = [sum(r["n"] for r in recs1[-1][k]) for k in ("bands", "bands_sampled", "bands_unsampled")]
    assert n[0] == n[1] + n[2]


def test_ring_ensemble_metrics_report(dev):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    image, coords, shape = make_kspace(*SHAPE)
    radii = [0.0, 0.5, 1.0, 5.0]
    tr = RingEnsembleTrainer(_cfg(batch_size=SHAPE[1] * SHAPE[2]), image, coords, shape, dev, radii=radii, seed=5)
    tr.fit(3)
    assert set(tr.metrics()) == {"psnr", "ssim"}
    tr.enable_band_report()
    m = tr.metrics()
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    want = B.band_report(B.band_stats_numpy(dist, image, tr.predict_all().cpu(),
                                            bounds=[(radii[i], radii[i + 1]) for i in range(3)]))
    _assert_report(m["bands"], want, dist.numel())


def test_reconstructor_compare_report(dev, tmp_path):
    from inr_mi355x.grid import GridSpec, grid_coords, grid_rows_numpy
    from inr_mi355x.reconstruct import Reconstructor
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    Cc, H, W = SHAPE
    image, _, shape = make_kspace(Cc, H, W)
    cfg = _cfg()
    tr = INRTrainer(cfg, image, grid_coords(Cc, H, W, device=dev), shape, dev, seed=3)
    tr.fit(2)
    path = str(tmp_path / "m.pt")
    torch.save(tr.checkpoint(), path)
    rec = Reconstructor(cfg, path, shape=SHAPE, device=dev)
    pred = rec.render()
    assert set(rec.compare(pred, image)) == {"psnr", "ssim"}
    dist = grid_rows_numpy(GridSpec(Cc, H, W), 0, Cc * H * W)[1]
    for arg, bounds in ((True, B.ring_bounds(8)), (5, B.ring_bounds(5)), ([(0.0, 0.4), (0.3, 5.0)],) * 2):
        out = rec.compare(pred, image, bands=arg)
        assert set(out) == {"psnr", "ssim", "bands"}
        want = B.band_report(B.band_stats_numpy(dist, image, pred.reshape(-1, 2).cpu(), bounds=bounds))
        _assert_report(out["bands"], want, dist.size)


def test_too_many_bands_are_refused_when_the_report_is_enabled(dev):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(*SHAPE)
    tr = INRTrainer(_cfg(partition=dict(no_steps=70, no_models=3)), image, coords, shape, dev, seed=3)
    for bounds in (None, 65, [(0.0, 1.0)] * 65, [(0.5, 0.25)]):
        with pytest.raises(ValueError):
            tr.enable_band_report(bounds)
    assert "bands" not in tr.metrics()
    tr.enable_band_report(64)
    assert len(tr.metrics()["bands"]) == 64


def test_multiscale_trainer_report(dev):
    """The multiscale trainer reports against the dist it was given (the one its heads are bounded by)."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    image, coords, shape = make_kspace(*SHAPE)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    cfg = _cfg(model="MultiscaleKFourier", lr=3e-4,
               net=dict(network_input_size=32, network_output_size=2, network_depth=8, network_width=32))
    tr = MultiscaleTrainer(cfg, image, coords, dist, [0.0, 0.4, 0.8, 1.2, 5.0], shape, dev, seed=1)
    tr.fit(2)
    assert "bands" not in tr.validate(0)
    tr.enable_band_report()
    rec = tr.validate(1)
    want = B.band_report(B.band_stats_numpy(dist, image, tr.predict_all().cpu(), bounds=B.ring_bounds(8)))
    _assert_report(rec["bands"], want, dist.numel())


def test_hp_search_keeps_the_best_validations_bands(dev, tmp_path):
    import json
    import os
    from inr_mi355x import hp_search as HS
    from conftest import GOLDEN
    base = dict(json.load(open(os.path.join(GOLDEN, "hp_search.json")))["base_config"], log_iter=1000)
    hp = {"method": "grid", "max_epoch": 2, "search_space": {"lr": {"values": [1e-4, 1e-3], "type": "item"}}}
    for sub in ("a", "b"):
        os.makedirs(tmp_path / sub)
    plain = HS.run_search(base, hp, str(tmp_path / "a"), synthetic=SHAPE)
    res = HS.run_search(base, hp, str(tmp_path / "b"), synthetic=SHAPE, band_report=5)
    rows = json.load(open(tmp_path / "b" / "results.json"))["results"]
    assert len(rows) == 2 and all(len(r["bands"]) == 5 and r["bands"][0]["n"] > 0 for r in rows)
    assert all("bands" not in r for r in plain["results"])
    for a, b in zip(plain["results"], res["results"]):  # the report changes no statistic
        assert all(a[k] == b[k] for k in ("best_psnr", "best_psnr_ep", "best_ssim", "best_ssim_ep"))
