"""The conventional baseline of an off-grid fit on the MI355X (config['trajectory_baseline']):
trajectory.cg_baseline -- conjugate gradients on A^H W A x = A^H W y with A = inr_nudft and A^H W = inr_adjoint_nudft --
against its fp64 restatement, and the record INRTrainer makes of it."""
import math

import numpy as np
import pytest
import torch

from inr_mi355x import trajectory as T
from inr_mi355x.evalchain import ifft2c, image_metrics
from inr_mi355x.synthetic import make_kspace
from inr_mi355x.train import INRTrainer

pytestmark = pytest.mark.gpu

SHAPE = (2, 32, 32)
SPOKES = 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scan():
    return make_kspace(*SHAPE)


def _complex(t):
    return torch.view_as_complex(t.cpu().contiguous()).numpy().astype(np.complex128)


@pytest.fixture(scope="module")
def samples(scan, dev):
    """(device samples [C, M, 2], their fp64 copy, positions, ramp weights) of spokes-12 on the synthetic scan"""
    image, _, shape = scan
    C, H, W = shape
    pos = T.spokes(H, W, SPOKES)
    y = T.nudft(ifft2c(image.reshape(C, H, W, 2).to(dev)).contiguous(), pos)
    return y, _complex(y), pos, T.density_ramp(SPOKES, 32, H, W)


def _objective(x, y64, pos, w):
    return float((w[None, :] * np.abs(T.nudft_numpy(x, pos) - y64) ** 2).sum())


def test_cg_objective_falls_as_in_fp64(samples):
    """4 iterations.  The fp64 objective of each device iterate, evaluated by numpy, is non-increasing (the fp64 ratios
    are >= 1.6, so fp32 rounding cannot reorder them), and the device's f_4 is <= numpy's f_3 -- a margin of 2.96 x taken
    from the fp64 run alone."""
    y, y64, pos, w = samples
    C, H, W = SHAPE
    iterates, objective = T.cg_baseline(y, pos, SHAPE, w, 4)
    assert len(iterates) == 4 and len(objective) == 5
    assert all(x.shape == (C, H, W, 2) and x.dtype == torch.float32 and x.is_cuda for x in iterates)
    _, f64 = T.cg_baseline_numpy(y64, pos, SHAPE, w, 4)
    f = [float((w[None, :] * np.abs(y64) ** 2).sum())] + [_objective(_complex(x), y64, pos, w) for x in iterates]
    print("fp64 objective of the device iterates:", ", ".join("%.6g" % v for v in f))
    print("fp64 run:                             ", ", ".join("%.6g" % v for v in f64))
    print("the device's own record:              ", ", ".join("%.6g" % v for v in objective))
    assert all(f[i + 1] <= f[i] for i in range(4))
    assert f[4] <= f64[3]
    assert all(math.isfinite(v) for v in objective) and all(objective[i + 1] <= objective[i] for i in range(4))


def test_zero_iterations_is_the_weighted_adjoint(samples):
    y, y64, pos, w = samples
    iterates, objective = T.cg_baseline(y, pos, SHAPE, w, 0)
    assert len(iterates) == 1 and len(objective) == 1 and math.isfinite(objective[0])
    want = T.nudft_adjoint(y, pos, SHAPE, w)
    assert torch.equal(iterates[0].view(torch.int32), want.view(torch.int32))


def test_one_iteration_on_the_full_grid_is_the_inverse_fft(scan, dev):
    """With every integer grid point as a position and uniform weights (w = 1) A is unitary: A^H W A = I, alpha = 1 and
    one iteration returns x_1 = A^H y = ifft2c(y).  The device applies three operators on the way: b = A^H y (error per
    pixel <= e = adjoint_error_bound(y)), q = A b and A^H q for the residual (not part of x_1).  x_1 = alpha b with
    alpha = <b, b> / <q, q>_w: the forward call's error on q (relative 2^-24 (H W + 32) in the worst case, like e relative
    to sum |y|) moves alpha by at most twice that, and |b| <= sum |y| / sqrt(H W) per pixel, so alpha's share is <= 2 e
    again; hipFFT's own error is inside e (test_gpu_adjoint_nudft).  Tolerance: 4 adjoint_error_bound."""
    image, _, shape = scan
    C, H, W = shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pos = np.stack([yy.ravel(), xx.ravel()], axis=1)
    k = image.reshape(C, H, W, 2).to(dev).contiguous()
    w = T.normalise_density(np.ones(H * W), H, W)
    assert np.array_equal(w, np.ones(H * W))
    iterates, objective = T.cg_baseline(k.reshape(C, H * W, 2), pos, shape, w, 1)
    got, want = _complex(iterates[0]), _complex(ifft2c(k))
    bound = T.adjoint_error_bound(_complex(k).reshape(C, -1), w, H, W)
    share = (np.abs(got - want) / bound[:, None, None]).max()
    print("max |x_1 - ifft2c(y)| / adjoint_error_bound = %.4f (allowed: 4)" % share)
    assert share <= 4.0
    assert objective[1] <= 1e-6 * objective[0]  # the data are reproduced: fp32 noise against sum |y|^2


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=500, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               val_epoch=1, encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               trajectory="spokes-%d" % SPOKES)
    cfg.update(kw)
    return cfg


def test_trainer_records_the_baseline(scan, dev):
    image, coords, shape = scan
    C, H, W = shape
    tr = INRTrainer(_cfg(trajectory_baseline="cg-4"), image, coords, shape, dev, seed=3)
    tr.fit(log_every=1)
    rec = tr.validate(1)
    g = rec["gridding"]
    assert set(g) == {"mode", "iters", "density", "psnr", "ssim", "objective", "seconds"}
    assert g["mode"] == "cg" and g["iters"] == 4 and g["density"] == "ramp"
    assert all(math.isfinite(g[k]) for k in ("psnr", "ssim", "seconds")) and g["seconds"] >= 0.0
    assert len(g["objective"]) == 5 and all(math.isfinite(v) for v in g["objective"])
    assert all(g["objective"][i + 1] <= g["objective"][i] for i in range(4))
    print("gridding: %.4f dB / SSIM %.4f; fit after 2 epochs: %.4f dB" % (g["psnr"], g["ssim"], rec["psnr"]))
    assert tr.metrics()["gridding"] == g and tr.gridding is g
    # the score is the validation's metric kernel applied to the returned image
    ref_rss = image_metrics(None, ifft2c(image.reshape(C, H, W, 2).to(dev)).contiguous())[0]
    assert tr.gridding_image.shape == (C, H, W, 2)
    m = image_metrics(ref_rss, tr.gridding_image)[1][:2].cpu().tolist()
    assert g["psnr"] == m[0] and g["ssim"] == m[1]
    # ... of the samples the fit trains on
    want = T.cg_baseline(tr.train_values, T.spokes(H, W, SPOKES), shape, T.density_ramp(SPOKES, 32, H, W), 4)[0][-1]
    assert torch.equal(tr.gridding_image.view(torch.int32), want.view(torch.int32))
    # the rest of the record, and the fit itself, are those of the fit without the switch
    assert rec["trajectory"] == tr.trajectory_info == {"kind": "spokes", "spokes": SPOKES, "readout": 32,
                                                       "rows_per_coil": SPOKES * 32, "acceleration": H * W / (SPOKES * 32)}
    plain = INRTrainer(_cfg(), image, coords, shape, dev, seed=3)
    plain.fit(log_every=1)
    assert torch.equal(tr.engine.params.view(torch.int32), plain.engine.params.view(torch.int32))
    rp = plain.validate(1)
    assert "gridding" not in rp and "gridding" not in plain.metrics() and plain.gridding is None
    assert {k: v for k, v in rec.items() if k != "gridding"} == rp
    # the plain adjoint
    adj = INRTrainer(_cfg(trajectory_baseline="adjoint", trajectory_density="uniform"), image, coords, shape, dev, seed=3)
    assert adj.gridding["mode"] == "adjoint" and adj.gridding["iters"] == 0 and adj.gridding["density"] == "uniform"
    assert len(adj.gridding["objective"]) == 1 and adj.gridding["psnr"] < g["psnr"]


def test_save_images_writes_the_gridding_picture(scan, dev, tmp_path):
    """--save-images: cli_folders, which writes the training pictures, writes the baseline's next to them"""
    import argparse
    import os
    from inr_mi355x.cli import cli_folders
    from inr_mi355x.display import read_png_gray
    image, coords, shape = scan
    C, H, W = shape
    tr = INRTrainer(_cfg(trajectory_baseline="cg-4", max_epoch=1), image, coords, shape, dev, seed=3)
    _, image_dir = cli_folders(tr, argparse.Namespace(output_path=str(tmp_path), save_images=True))
    g = tr.gridding
    path = os.path.join(image_dir, "gridding_{:.4g}_psnr_{:.4g}_ssim.png".format(g["psnr"], g["ssim"]))
    assert os.path.isfile(path)
    px = read_png_gray(path)
    assert tuple(px.shape) == (H, W) and int(px.max()) > int(px.min())
