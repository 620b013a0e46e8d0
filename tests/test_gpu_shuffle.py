"""Shuffled epochs on the MI355X (``-m gpu``): inr_shuffle_epoch against the numpy restatement of DESIGN.md section 4.12
(exact: integers and copies), and shuffled fits of the three trainers against a loop built from the oracle's public
parts over ``coords[order_e]`` / ``image[order_e]`` with ``order_e = epoch_order(n, seed, e)``.

Tolerances of the trajectory checks are the ones the sequential trajectory tests hold the same models to against the
oracle: per-step losses rtol 5e-5 (test_gpu_parity.py test_logf_encoder_and_trainer / ring ensemble, test_gpu_mfn.py
test_single_scale_trainer_mfn_vs_oracle, multiscale), final outputs rtol 1e-3 + atol 2e-5.  Measured margins:
profiles/shuffle_parity_errors.jsonl (record_parity).
"""
import numpy as np
import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402  (checker only)

N_LIST = [1, 2, 3, 255, 256, 257, 25000, 15 * 640 * 368]
LOSS_RTOL = 5e-5
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)
ENC = dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3)
HDR_OPTS = dict(hdr_eps=1e-3, hdr_ff_sigma=2.0, hdr_ff_factor=0.5)  # the trainers' defaults, spelled out for the oracle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---- the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_LIST)
def test_order_equals_host_restatement(dev, n):
    from inr_mi355x.shuffle import device_order, epoch_order
    for seed, epoch in ((0, 0), (0, 1), (7, 0), (2 ** 40 + 3, 12), (2 ** 64 - 1, 2 ** 32 - 1)):
        got = device_order(n, seed, epoch, dev).cpu().numpy()
        want = epoch_order(n, seed, epoch)
        assert got.dtype == want.dtype == np.int64
        assert np.array_equal(got, want), (n, seed, epoch)


@pytest.mark.parametrize("n,bs", [(1, 1), (3, 2), (257, 64), (257, 100), (25000, 777), (25000, 25000), (25000, 30000),
                                  (15 * 640 * 368, 25000)])
@pytest.mark.parametrize("with_mask", [False, True])
def test_gather_and_batch_counts(dev, n, bs, with_mask):
    from inr_mi355x.shuffle import epoch_order, shuffle_epoch
    g = torch.Generator().manual_seed(n + bs)
    coords, gt, dist = torch.rand(n, 3, generator=g), torch.randn(n, 2, generator=g), torch.rand(n, generator=g)
    mask = (torch.rand(n, generator=g) < 0.37).to(torch.uint8) if with_mask else None
    nb = -(-n // bs)
    d = dict(coords=coords.to(dev), gt=gt.to(dev), dist=dist.to(dev), mask=None if mask is None else mask.to(dev))
    out = dict(coords_out=torch.full((n, 3), -7.0, device=dev), gt_out=torch.full((n, 2), -7.0, device=dev),
               dist_out=torch.full((n,), -7.0, device=dev),
               mask_out=torch.full((n,), 9, dtype=torch.uint8, device=dev) if with_mask else None)
    counts = torch.full((nb,), -5, dtype=torch.int32, device=dev)
    order_out = torch.empty(n, dtype=torch.int64, device=dev)
    seed, epoch = 11, 3
    shuffle_epoch(n, seed, epoch, dev, **d, **out, batch_size=bs, batch_counts=counts, order_out=order_out)
    order = torch.from_numpy(epoch_order(n, seed, epoch))
    assert torch.equal(order_out.cpu(), order)
    assert torch.equal(out["coords_out"].cpu(), coords[order])
    assert torch.equal(out["gt_out"].cpu(), gt[order])
    assert torch.equal(out["dist_out"].cpu(), dist[order])
    flags = torch.ones(n, dtype=torch.int64) if mask is None else mask[order].to(torch.int64)
    if mask is not None:
        assert torch.equal(out["mask_out"].cpu(), mask[order])
    want = [int(flags[b * bs:(b + 1) * bs].sum()) for b in range(nb)]
    assert counts.cpu().tolist() == want
    # a second call into the same buffers gives the same result (the counts are zeroed by the call, not by the caller)
    shuffle_epoch(n, seed, epoch, dev, **d, **out, batch_size=bs, batch_counts=counts)
    assert counts.cpu().tolist() == want


def test_wrapper_refuses_bad_buffers(dev):
    from inr_mi355x.shuffle import shuffle_epoch
    n = 100
    c, co = torch.zeros(n, 3, device=dev), torch.zeros(n, 3, device=dev)
    with pytest.raises(RuntimeError, match="shape"):
        shuffle_epoch(n, 0, 0, dev, coords=c, coords_out=torch.zeros(n - 1, 3, device=dev))
    with pytest.raises(RuntimeError, match="contiguous"):
        shuffle_epoch(n, 0, 0, dev, coords=c.double(), coords_out=co)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shuffle_epoch(n, 0, 0, dev, coords=c.cpu(), coords_out=co)
    with pytest.raises(RuntimeError, match="go together"):
        shuffle_epoch(n, 0, 0, dev, coords=c)
    with pytest.raises(RuntimeError, match="in-place"):
        shuffle_epoch(n, 0, 0, dev, coords=c, coords_out=c)
    with pytest.raises(RuntimeError, match="batch_size"):
        shuffle_epoch(n, 0, 0, dev, batch_counts=torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="no output"):
        shuffle_epoch(n, 0, 0, dev)


# ---- trainers against a loop over the permuted rows, built from the oracle's public parts -----------------------------
def _oracle_shuffled_loop(cfg, sd, enc_B, coords, image, seed, max_steps, mask=None, dist=None, radii=None):
    """train.py:158-192 (train_kspace_multiscale.py:164-195 when ``radii`` is given) with the rows of epoch e taken in
    the order epoch_order(n, seed, e): O.encode, O.model_forward, O.make_loss / the multiscale terms, O.adam_init,
    O.adam_step, O.lr_factor.  Mutates ``sd``; returns the per-step losses."""
    from inr_mi355x.shuffle import epoch_order
    model = {"Fourier": "MultiscaleKFourier"}.get(cfg["model"], cfg["model"]) if radii is not None else cfg["model"]
    keys = O.trainable_keys(model, sd)
    params = {k: sd[k].requires_grad_(True) for k in keys}
    state = O.adam_init(params)
    loss_fn = O.make_loss(cfg) if radii is None else None
    n, bs = coords.shape[0], cfg["batch_size"]
    losses = []
    for epoch in range(cfg["max_epoch"]):
        order = torch.from_numpy(epoch_order(n, seed, epoch))
        c_e, i_e = coords[order], image[order]
        m_e = None if mask is None else mask[order]
        d_e = None if dist is None else dist[order]
        lr = cfg["lr"] * O.lr_factor(epoch, cfg["max_epoch"])
        for lo in range(0, n, bs):
            if len(losses) >= max_steps:
                break
            hi = min(lo + bs, n)
            kc, gt = c_e[lo:hi], i_e[lo:hi]
            x = O.encode(kc, enc_B, cfg["encoder"]["embedding"])
            if radii is None:
                out = O.model_forward(model, sd, x, cfg["net"])
                if m_e is not None:
                    out, gt = out[m_e[lo:hi]], gt[m_e[lo:hi]]
                loss = loss_fn(out, gt, kc)
            else:
                d = d_e[lo:hi]
                outs = O.model_forward(model, sd, x, cfg["net"], dist_to_center=d, boundaries=O.create_pairs(radii, 2))
                loss = 0.1 * O.loss_consistency(outs, d, O.create_pairs(radii, 1))
                if m_e is not None:
                    gt = gt[m_e[lo:hi]]
                for out in outs:
                    if m_e is not None:
                        out = out[m_e[lo:hi]]
                    loss = loss + {"L2": O.loss_l2_half, "L1": O.loss_l1_half}[cfg["loss"]](out, gt)
            grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
            with torch.no_grad():
                O.adam_step(params, dict(zip(keys, grads)), state, lr, cfg["beta1"], cfg["beta2"], 1e-8,
                            cfg["weight_decay"])
            losses.append(float(loss.detach()))
    for k in keys:
        sd[k].requires_grad_(False)
    return losses


def _cfg(model, loss, **kw):
    cfg = dict(model=model, loss=loss, lr=1e-3, batch_size=300, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               net=dict(NET, network_width=48) if model != "SIREN" else dict(NET), encoder=dict(ENC), shuffle=True,
               loss_opts=dict(HDR_OPTS))
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("model", ["SIREN", "Fourier"])
@pytest.mark.parametrize("loss", ["L2", "HDR"])
@pytest.mark.parametrize("masked", [False, True])
def test_shuffled_trajectory_vs_oracle_parts(dev, model, loss, masked):
    """Two shuffled epochs (4 batches each, the last one short) of INRTrainer: losses and final outputs."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    C, H, W = 2, 24, 20
    image, coords, shape = make_kspace(C, H, W)
    cfg = _cfg(model, loss, shuffle_seed=9)
    mask = (torch.rand(coords.shape[0], generator=torch.Generator().manual_seed(2)) < 0.7) if masked else None
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3, mask=mask)
    assert tr.steps_per_epoch == 4
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    want = _oracle_shuffled_loop(cfg, sd, tr.encoder.B.cpu(), coords, image, 9, 8, mask=mask)
    got = np.array([s[1] for s in tr.fit(log_every=1)])
    assert len(got) == len(want) == 8
    err = float(np.max(np.abs(got - np.array(want)) / np.abs(np.array(want))))
    out = tr.predict_all().cpu()  # reads the unshuffled resident rows
    with torch.no_grad():
        ref = O.model_forward(model, sd, O.encode(coords, tr.encoder.B.cpu(), "gauss"), cfg["net"])
    record_parity("shuffled_trajectory", model=model, loss=loss, masked=masked, loss_rel_err=err,
                  out_abs_err=float((out - ref).abs().max()))
    np.testing.assert_allclose(got, np.array(want), rtol=LOSS_RTOL)
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=2e-5)
    # ... and the order matters: the sequential fit walks another trajectory
    seq = INRTrainer(dict(cfg, shuffle=False), image, coords, shape, dev, seed=3, mask=mask)
    assert not np.allclose(np.array([s[1] for s in seq.fit(log_every=1)]), got, rtol=1e-3)


def _fit_params(cfg, image, coords, shape, dev, mask=None, steps=None):
    from inr_mi355x.train import INRTrainer
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3, mask=mask)
    losses = [float(s[1]) for s in tr.fit(steps, log_every=1)]
    return tr.engine.params.clone(), losses


def test_shuffle_off_is_bitwise_the_default(dev):
    from inr_mi355x.synthetic import make_kspace
    image, coords, shape = make_kspace(2, 24, 20)
    mask = torch.rand(coords.shape[0], generator=torch.Generator().manual_seed(2)) < 0.7
    for loss in ("L2", "HDR"):
        cfg = _cfg("SIREN", loss)
        del cfg["shuffle"]
        p0, l0 = _fit_params(cfg, image, coords, shape, dev, mask)
        p1, l1 = _fit_params(dict(cfg, shuffle=False, shuffle_seed=5), image, coords, shape, dev, mask)
        assert torch.equal(p0, p1) and l0 == l1


def test_same_seed_same_fit_and_resume(dev, tmp_path):
    """Two runs with one seed agree bitwise; another seed does not; a fit checkpointed after epoch 1 and resumed through
    config['pretrain'] ends epoch 3 where the uninterrupted fit does, bitwise (the order is a function of the epoch)."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 24, 20)
    cfg = _cfg("SIREN", "HDR", max_epoch=4, shuffle_seed=21)
    p0, l0 = _fit_params(cfg, image, coords, shape, dev)
    p1, l1 = _fit_params(cfg, image, coords, shape, dev)
    assert torch.equal(p0, p1) and l0 == l1
    p2, _ = _fit_params(dict(cfg, shuffle_seed=22), image, coords, shape, dev)
    assert not torch.equal(p0, p2)
    a = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    for epoch in range(2):
        for it in range(a.steps_per_epoch):
            a.step(epoch, it)
    ck = a.checkpoint()
    assert set(ck) == {"net", "enc", "opt"}
    path = str(tmp_path / "ck.pt")
    torch.save(ck, path)
    b = INRTrainer(dict(cfg, pretrain=path), image, coords, shape, dev, seed=99)
    tail = []
    for epoch in range(2, 4):
        for it in range(b.steps_per_epoch):
            tail.append(float(b.step(epoch, it)))
    assert torch.equal(b.engine.params, p0)
    assert tail == l0[2 * a.steps_per_epoch:]


def test_shuffle_reads_counts_once_per_epoch(dev, monkeypatch):
    """The epoch boundary is one kernel call and one read-back; the steps in between make neither."""
    from inr_mi355x import shuffle as S
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 24, 20)
    calls = []
    real = S.shuffle_epoch
    monkeypatch.setattr(S, "shuffle_epoch", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    tr = INRTrainer(_cfg("SIREN", "L2", max_epoch=3), image, coords, shape, dev, seed=3)
    tr.fit()
    assert calls == [0, 1, 2] and tr.global_step == 12


def test_center_loss_with_shuffle(dev):
    """'LSL' (CenterLoss) on plain single-rank batches: the pair rows come from the epoch buffer's coordinates."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 24, 20)
    cfg = _cfg("SIREN", "LSL", loss_opts=dict(HDR_OPTS, min_sample=40), shuffle_seed=4)
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    torch.manual_seed(77)
    got = np.array([s[1] for s in tr.fit(log_every=1)])
    torch.manual_seed(77)
    want = _oracle_shuffled_loop(cfg, sd, tr.encoder.B.cpu(), coords, image, 4, 8)
    record_parity("shuffled_center_loss", loss_rel_err=float(np.max(np.abs(got - want) / np.abs(want))))
    np.testing.assert_allclose(got, np.array(want), rtol=LOSS_RTOL)


def test_ring_ensemble_shuffled_vs_oracle_parts(dev):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    C, H, W = 2, 40, 32
    image, coords, shape = make_kspace(C, H, W)
    cfg = dict(model="SIREN", loss="L2", lr=2e-4, batch_size=1000, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               partition=dict(no_steps=20, no_models=3), net=dict(NET), encoder=dict(ENC), shuffle=True, shuffle_seed=6)
    tr = RingEnsembleTrainer(cfg, image, coords, shape, dev, seed=5)
    sds = {i: {k: v.detach().cpu().clone() for k, v in tr.models[i].state_dict().items()} for i in tr.owned}
    logged = tr.fit(log_every=1)
    assert len(logged) == 2 * 3
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    for i in range(3):
        # uniform batches of 1000 rows hold rows of every ring, so no ring's optimizer step is ever skipped
        mask = (dist >= tr.radii[i]) & (dist <= tr.radii[i + 1])
        want = _oracle_shuffled_loop(cfg, sds[i], tr.encoder.B.cpu(), coords, image, 6, 6, mask=mask)
        got = np.array([l[1][i] for l in logged], dtype=float)
        record_parity("shuffled_ring_ensemble", ring=i, loss_rel_err=float(np.max(np.abs(got - want) / np.abs(want))))
        np.testing.assert_allclose(got, np.array(want), rtol=LOSS_RTOL, err_msg=f"ring {i}")
    assert np.isfinite(tr.evaluate())


@pytest.mark.parametrize("masked", [False, True])
def test_multiscale_shuffled_vs_oracle_parts(dev, masked):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    C, H, W = 2, 24, 20
    image, coords, shape = make_kspace(C, H, W)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    radii = [0.0, 0.4, 0.8, 1.2, 5.0]
    cfg = dict(model="MultiscaleKFourier", loss="L2", lr=3e-4, batch_size=300, max_epoch=2, weight_decay=0.0, beta1=0.9,
               beta2=0.999, net=dict(network_input_size=32, network_output_size=2, network_depth=8, network_width=32),
               encoder=dict(ENC), shuffle=True, shuffle_seed=13)
    mask = (torch.rand(coords.shape[0], generator=torch.Generator().manual_seed(4)) < 0.6) if masked else None
    img = image if mask is None else image * mask[:, None]
    tr = MultiscaleTrainer(cfg, img, coords, dist, radii, shape, dev, seed=1, mask=mask)
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    want = _oracle_shuffled_loop(cfg, sd, tr.encoder.B.cpu(), coords, img, 13, 8, mask=mask, dist=dist, radii=radii)
    got = np.array([s[1] for s in tr.fit(log_every=1)])
    record_parity("shuffled_multiscale", masked=masked, loss_rel_err=float(np.max(np.abs(got - want) / np.abs(want))))
    np.testing.assert_allclose(got, np.array(want), rtol=LOSS_RTOL)


def test_percoil_tv_shuffled_coil_order(dev):
    """per_coil + TV + shuffle: the batches stay whole coils (views of the resident grid), visited in
    epoch_order(C, seed, epoch); against the oracle's per-coil step taken in that order."""
    from inr_mi355x.shuffle import coil_order
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    C, H, W = 5, 16, 12
    image, coords, shape = make_kspace(C, H, W)
    mask = torch.rand(C * H * W, generator=torch.Generator().manual_seed(8)) < 0.5
    img = image * mask[:, None]
    cfg = dict(_cfg("SIREN", "L2", max_epoch=2, shuffle_seed=17), per_coil=True, use_tv=True)
    tr = INRTrainer(cfg, img, coords, shape, dev, seed=3, mask=mask)
    assert tr.use_tv and tr.bs == H * W
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    got = np.array([s[1] for s in tr.fit(log_every=1)])
    # the oracle's loop over the coils in the permuted order, one epoch at a time (its own per-epoch learning rate)
    keys = O.trainable_keys("SIREN", sd)
    params = {k: sd[k].requires_grad_(True) for k in keys}
    state, loss_fn, want = O.adam_init(params), O.make_loss(cfg), []
    for epoch in range(2):
        order = coil_order(C, 17, epoch)
        assert sorted(order) == list(range(C))
        lr = cfg["lr"] * O.lr_factor(epoch, cfg["max_epoch"])
        for c in order:
            lo, hi = c * H * W, (c + 1) * H * W
            out = O.model_forward("SIREN", sd, O.encode(coords[lo:hi], tr.encoder.B.cpu(), "gauss"), cfg["net"])
            loss = O.loss_tv(out.view(H, W, 2)) + loss_fn(out[mask[lo:hi]], img[lo:hi][mask[lo:hi]], coords[lo:hi])
            grads = torch.autograd.grad(loss, list(params.values()))
            with torch.no_grad():
                O.adam_step(params, dict(zip(keys, grads)), state, lr, cfg["beta1"], cfg["beta2"], 1e-8, 0.0)
            want.append(float(loss.detach()))
    record_parity("shuffled_percoil_tv", loss_rel_err=float(np.max(np.abs(got - want) / np.abs(want))))
    np.testing.assert_allclose(got, np.array(want), rtol=LOSS_RTOL)
    assert coil_order(C, 17, 0) != coil_order(C, 17, 1)


def test_iter_batches_shuffled(dev):
    from inr_mi355x.datasets import iter_batches
    from inr_mi355x.shuffle import epoch_order
    from inr_mi355x.synthetic import make_kspace

    class DS:
        def __init__(self, coords, image):
            self.coords, self.image = coords, image

        def __getitem__(self, idx):
            return self.coords[idx], self.image[idx], list(), list()

        def __len__(self):
            return len(self.image)

    image, coords, _ = make_kspace(2, 24, 20)
    ds = DS(coords.to(dev), image.to(dev))
    seq = list(iter_batches(ds, 300))
    assert torch.equal(torch.cat([b[0] for b in seq]).cpu(), coords)
    order = torch.from_numpy(epoch_order(len(ds), 5, 2))
    got = list(iter_batches(ds, 300, shuffle_seed=5, epoch=2))
    assert [len(b[0]) for b in got] == [300, 300, 300, 60]
    assert torch.equal(torch.cat([b[0] for b in got]).cpu(), coords[order])
    assert torch.equal(torch.cat([b[1] for b in got]).cpu(), image[order])
