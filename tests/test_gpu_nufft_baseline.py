"""config['trajectory_operator'] on the MI355X: the conventional baseline of an off-grid fit with
the Kaiser-Bessel pair inside (trajectory.cg_baseline(operator="gridding")) next to the exact pair, and the switch in
INRTrainer -- which selects the baseline's operator only: the training samples, and so the fit, stay as they are."""
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
# |f_gridding - f_exact| / f_exact of the fp64 objective after iterations 1..4 (test_nufft_host.CG_MEASURED), times 4
CG_MARGIN = [4 * v for v in (3.039e-06, 8.599e-07, 3.380e-06, 1.067e-06)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scan():
    return make_kspace(*SHAPE)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=500, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               trajectory="spokes-%d" % SPOKES)
    cfg.update(kw)
    return cfg


def test_the_fit_is_the_same_and_the_record_names_the_operator(scan, dev):
    image, coords, shape = scan
    fits = {}
    for name, extra in (("gridding", dict(trajectory_operator="gridding")), ("absent", {}),
                        ("exact", dict(trajectory_operator="exact"))):
        tr = INRTrainer(_cfg(trajectory_baseline="cg-4", **extra), image, coords, shape, dev, seed=3)
        tr.fit(max_steps=3, log_every=0)
        torch.cuda.synchronize()
        fits[name] = tr
    a, b = fits["gridding"].engine, fits["absent"].engine
    for x, y in ((a.params, b.params), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert fits["gridding"].global_step == 3
    assert torch.equal(fits["gridding"].train_values.view(torch.int32), fits["absent"].train_values.view(torch.int32))
    assert fits["gridding"].gridding["operator"] == "gridding" and fits["exact"].gridding["operator"] == "exact"
    # the key absent: the exact pair, and nothing new recorded
    assert fits["absent"].trajectory_operator is None and "operator" not in fits["absent"].gridding
    assert torch.equal(fits["absent"].gridding_image.view(torch.int32), fits["exact"].gridding_image.view(torch.int32))
    assert fits["gridding"].metrics()["gridding"]["operator"] == "gridding"
    g, e = fits["gridding"].gridding, fits["exact"].gridding
    assert set(g) == set(e) == {"mode", "iters", "density", "psnr", "ssim", "objective", "seconds", "operator"}
    print("cg-4: gridding %.4f dB / %.4f, exact %.4f dB / %.4f" % (g["psnr"], g["ssim"], e["psnr"], e["ssim"]))
    # the image is the library call's
    want = T.cg_baseline(fits["gridding"].train_values, T.spokes(32, 32, SPOKES), shape, T.density_ramp(SPOKES, 32, 32, 32),
                         4, operator="gridding")[0][-1]
    assert torch.equal(fits["gridding"].gridding_image.view(torch.int32), want.view(torch.int32))


def test_cg4_under_gridding_against_exact(scan, dev):
    """Objective: the two fp64 runs differ by CG_MARGIN per iterate (measured, x 4); each device run differs from its own
    fp64 run by fp32 rounding.  The objective is f = sum w |A x - y|^2 with A x carried along; a perturbation d of A x
    per sample moves f by at most 2 sqrt(f) sqrt(sum w d^2) + sum w d^2.  d is bounded per operator call by the forward
    bounds (nufft_error_bound / error_bound of the iterate), and CG applies the operator once per iteration, so after
    k iterations d <= k max-bound (the step lengths are O(1): sum w = H W makes A^H W A of unit scale).
    PSNR: 10 log10(max / mse); the two images differ per pixel by at most the approximation error 4 x 2.998e-06 x
    sum |w y| / sqrt(H W) per adjoint call plus the rounding bounds, accumulated over the 4 iterations."""
    image, _, shape = scan
    C, H, W = shape
    pos, w = T.spokes(H, W, SPOKES), T.density_ramp(SPOKES, 32, H, W)
    coil = ifft2c(image.reshape(C, H, W, 2).to(dev)).contiguous()
    y = T.nudft(coil, pos)
    it_e, f_e = T.cg_baseline(y, pos, shape, w, 4)
    it_g, f_g = T.cg_baseline(y, pos, shape, w, 4, operator="gridding")
    assert len(it_g) == 4 and len(f_g) == 5 and f_g[0] == f_e[0]
    assert all(x.shape == (C, H, W, 2) and x.dtype == torch.float32 and x.is_cuda for x in it_g)
    wsum = float(w.sum())
    for k in range(1, 5):
        x_e = torch.view_as_complex(it_e[k - 1].cpu().contiguous()).numpy()
        x_g = torch.view_as_complex(it_g[k - 1].cpu().contiguous()).numpy()
        d = k * max(float(T.nufft_error_bound(x_g, pos).max()), float(T.error_bound(x_e, H, W).max()))
        rounding = sum(2.0 * math.sqrt(f) * math.sqrt(wsum) * d + wsum * d * d for f in (f_e[k], f_g[k]))
        margin = CG_MARGIN[k - 1] * f_e[k] + rounding
        print("iterate %d: f exact %.6g, gridding %.6g, |difference| / margin = %.4f"
              % (k, f_e[k], f_g[k], abs(f_g[k] - f_e[k]) / margin))
        assert abs(f_g[k] - f_e[k]) <= margin
    assert all(f_g[i + 1] <= f_g[i] for i in range(4))
    # PSNR of the two reconstructions against the full data
    ref_rss = image_metrics(None, coil)[0]
    p_e, p_g = (float(image_metrics(ref_rss, x[-1].contiguous())[1][0]) for x in (it_e, it_g))
    yw = (np.abs(torch.view_as_complex(y.cpu().contiguous()).numpy()) * w[None, :]).sum(axis=1)
    per_pixel = 4 * (4 * 2.998e-06 * yw / math.sqrt(H * W) + T.nufft_adjoint_error_bound(y.cpu(), pos, w, H, W)
                     + T.adjoint_error_bound(y.cpu(), w, H, W))
    rss_e = image_metrics(None, it_e[-1].contiguous())[0].double().cpu().numpy()
    mse = float(((rss_e - ref_rss.double().cpu().numpy()) ** 2).mean())
    d_rss = math.sqrt(float((per_pixel ** 2).sum()))  # RSS over coils of the per-pixel differences
    d_mse = 2.0 * math.sqrt(mse) * d_rss + d_rss ** 2
    margin_db = 10.0 / math.log(10.0) * d_mse / (mse - d_mse)
    print("PSNR exact %.5f dB, gridding %.5f dB, margin %.5f dB" % (p_e, p_g, margin_db))
    assert abs(p_g - p_e) <= margin_db


def test_the_key_without_a_baseline_is_refused(scan, dev):
    image, coords, shape = scan
    for extra in (dict(trajectory_operator="gridding"), dict(trajectory_operator="gridding", trajectory_baseline="none")):
        with pytest.raises(ValueError, match="trajectory_operator"):
            INRTrainer(_cfg(**extra), image, coords, shape, dev, seed=3)
    with pytest.raises(ValueError, match="trajectory_operator"):
        INRTrainer(_cfg(trajectory_baseline="cg-2", trajectory_operator="kaiser"), image, coords, shape, dev, seed=3)
