"""Off-grid fits on the MI355X (config['trajectory']): INRTrainer trains on the C*M samples of
golden-angle spokes taken from the resident k-space by inr_nudft and validates on the Cartesian grid."""
import math

import numpy as np
import pytest
import torch

from inr_mi355x import trajectory as T
from inr_mi355x.evalchain import ifft2c
from inr_mi355x.synthetic import make_kspace
from inr_mi355x.train import INRTrainer

pytestmark = pytest.mark.gpu

SHAPE = (2, 32, 32)
BS = 500  # C * M = 2 * 24 * 32 = 1536 = 3 * 500 + 36
EPOCHS = 20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scan():
    return make_kspace(*SHAPE)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=BS, max_epoch=EPOCHS, weight_decay=0.0, beta1=0.9, beta2=0.999,
               val_epoch=1, encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))
    cfg.update(kw)
    return cfg


def _fit(scan, dev, **kw):
    image, coords, shape = scan
    tr = INRTrainer(_cfg(**kw), image, coords, shape, dev, seed=3)
    return tr, tr.fit(log_every=1)


@pytest.fixture(scope="module")
def offgrid(scan, dev):
    return _fit(scan, dev, trajectory="spokes-24")


def test_training_rows_are_the_spokes(scan, dev, offgrid):
    tr, _ = offgrid
    image, _, shape = scan
    C, H, W = shape
    pos = T.spokes(H, W, 24)
    M = pos.shape[0]
    assert M == 24 * 32 and tr.n_train == C * M and tr.n == C * H * W
    assert tr.steps_per_epoch == math.ceil(C * M / BS) == 4 and (C * M) % BS != 0
    assert tr.trajectory_info == {"kind": "spokes", "spokes": 24, "readout": 32, "rows_per_coil": M,
                                  "acceleration": H * W / M}
    assert torch.equal(tr.train_coords.cpu(), T.trajectory_coords(pos, C, H, W))
    img = ifft2c(image.reshape(C, H, W, 2).to(dev)).cpu()  # the coil images the kernel was given
    want = T.nudft_numpy(img, pos)
    got = torch.view_as_complex(tr.train_values.cpu().reshape(C, M, 2).contiguous()).numpy().astype(np.complex128)
    bound = T.error_bound(img, H, W)
    print("train_values: max |out - ref| / bound = %.4f" % (np.abs(got - want) / bound[:, None]).max())
    assert (np.abs(got - want) <= bound[:, None]).all()
    # the centre sample of every spoke is a grid point: the resident k-space value itself
    grid = torch.view_as_complex(image.reshape(C, H, W, 2).contiguous()).numpy()
    centre = got.reshape(C, 24, 32)[:, :, 16]
    assert (np.abs(centre - grid[:, H // 2, W // 2][:, None]) <= 2 * bound[:, None]).all()
    # the grid data stay what validation reads
    assert torch.equal(tr.image_full.cpu(), image) and tr.coords.shape[0] == C * H * W


def test_loss_falls_and_validation_reads_the_grid(offgrid):
    tr, logged = offgrid
    n = tr.steps_per_epoch
    assert len(logged) == EPOCHS * n and tr.global_step == EPOCHS * n
    losses = [v for _, v in logged]
    first, last = sum(losses[:n]) / n, sum(losses[-n:]) / n
    print("mean logged loss: first epoch %.6g, last epoch %.6g" % (first, last))
    assert all(math.isfinite(v) for v in losses) and last < first
    rec = tr.validate(EPOCHS - 1)
    assert all(math.isfinite(rec[k]) for k in ("psnr", "ssim", "test_loss"))
    assert rec["trajectory"] == tr.trajectory_info and tr.metrics()["trajectory"] == tr.trajectory_info
    C, H, W = SHAPE
    pred = tr.predict_all()
    assert pred.shape == (C * H * W, 2)
    # PSNR on the 2 x 32 x 32 grid, as evaluate() forms it from the full data
    assert abs(rec["psnr"] - tr.evaluate()) <= 1e-3 * max(1.0, abs(rec["psnr"]))
    # the test loss: the grid's sequential batches of batch_size rows, summed, over the TRAINING loader's length
    total = 0.0
    for lo in range(0, C * H * W, BS):
        hi = min(lo + BS, C * H * W)
        loss, _ = tr.engine.loss_grad(tr.loss, pred[lo:hi], tr.image_full[lo:hi], hi - lo, hdr_A=0.0)
        total += float(loss)
    assert rec["test_loss"] == pytest.approx(total / tr.steps_per_epoch, rel=1e-6)
    assert set(tr.checkpoint()) == {"net", "enc", "opt"}


def test_shuffled_offgrid_fit_is_reproducible(scan, dev):
    a, la = _fit(scan, dev, trajectory="spokes-24", shuffle=True, max_epoch=3)
    b, lb = _fit(scan, dev, trajectory="spokes-24", shuffle=True, max_epoch=3)
    assert a.shuffle and a._epoch_buf is not None and a._epoch_buf.n == a.n_train
    assert len(la) == 3 * a.steps_per_epoch and la == lb and all(math.isfinite(v) for _, v in la)
    assert torch.equal(a.engine.params.view(torch.int32), b.engine.params.view(torch.int32))
    plain, lp = _fit(scan, dev, trajectory="spokes-24", max_epoch=3)
    assert la != lp  # the batches differ from the sequential ones


def test_hdr_loss_takes_the_training_rows(scan, dev):
    """the HDR scalar A of a training batch comes from the off-grid rows, validation's from the grid rows"""
    tr, logged = _fit(scan, dev, trajectory="spokes-24", loss="HDR", max_epoch=1)
    from inr_mi355x.train import hdr_weight
    lo, hi = tr._range(1)
    assert tr._hdr_A_train[1] == float(torch.mean(hdr_weight(tr.train_coords[lo:hi], tr.loss.sigma)))
    rec = tr.validate(0)
    assert math.isfinite(rec["test_loss"]) and len(tr._hdr_A) == math.ceil(tr.n / BS)
    assert tr._hdr_A[1] == float(torch.mean(hdr_weight(tr.coords[BS:2 * BS], tr.loss.sigma)))


def test_switch_off_is_the_grid_fit(scan, dev):
    """absent and "none" are the same fit, bit for bit, and carry nothing of the switch"""
    a, la = _fit(scan, dev, max_epoch=2)
    b, lb = _fit(scan, dev, trajectory="none", max_epoch=2)
    assert la == lb and torch.equal(a.engine.params.view(torch.int32), b.engine.params.view(torch.int32))
    ra, rb = a.validate(1), b.validate(1)
    assert ra == rb and "trajectory" not in ra and "trajectory" not in a.metrics()
    assert a.trajectory is None and a.n_train == a.n and a.train_coords is a.coords and a.train_values is a.image
    assert a.steps_per_epoch == math.ceil(a.n / BS)
