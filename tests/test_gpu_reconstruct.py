"""Reconstruction from a checkpoint on the MI355X (``-m gpu``): inr_mi355x/reconstruct.py against the trainers' own
prediction sweep (bit-equal on the grid the trainer was built on), against the engine's forward on the restated
coordinates (windows, coil subsets, other resolutions), its files, and the command line.

Tolerances: bit-equality wherever the same kernels see the same coordinates; the forward tolerance of
tests/test_gpu_parity.py (rtol 1e-5, atol 1e-6) where only the chunking differs; and, for a trainer built on the old
host grid (synthetic.create_coords, at most 2^-24 from the device grid per coordinate), ten times the deviation first
measured on the GPU -- a wrong axis or a swapped window is orders of magnitude above it (record_parity keeps the figures).
"""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT, record_parity

pytestmark = pytest.mark.gpu

SHAPE = (2, 24, 20)
ENC = dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3)
NONE_ENC = dict(embedding="none", scale=1, embedding_size=3, coordinates_size=3)
RADII = [0.0, 0.4, 0.8, 1.2, 5.0]
WINDOW = (-0.5, 0.25, 0.1, 0.7)
# First measured on the GPU (SIREN 3 x 32 after 2 steps, 2 x 24 x 20): the native reconstruction against predict_all() of a
# trainer on create_coords' grid, largest deviation relative to max|pred|; and the dB between the training command's PSNR
# and the reconstruction command's.  The tests bound both at ten times these values.
OLD_GRID_REL_DEV_MEASURED = 9.28e-7
CLI_PSNR_GAP_DB_MEASURED = 1.25e-6


def _mlp_net(n_in, width=32, depth=3, **kw):
    return dict(network_input_size=n_in, network_output_size=2, network_depth=depth, network_width=width, **kw)


def _config(case: str) -> dict:
    cfg = dict(loss="L2", lr=1e-3, batch_size=300, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               model=case, encoder=dict(ENC), net=_mlp_net(32))
    if case == "SIREN_LogF":
        cfg.update(model="SIREN", encoder=dict(embedding="LogF", scale=5, embedding_size=60, coordinates_size=3),
                   net=_mlp_net(60))
    elif case == "SIREN_image":
        cfg.update(model="SIREN", transform=True)
    elif case in ("WIRE", "WIRE2D"):
        cfg.update(encoder=dict(NONE_ENC), net=_mlp_net(3, first_omega_0=10, hidden_omega_0=10, scale=5))
    elif case in ("Fourier", "Gabor", "KGabor"):
        cfg.update(net=_mlp_net(32, width=48))
    elif case == "MultiscaleKFourier":
        cfg.update(lr=3e-4, net=_mlp_net(32, depth=8))
    return cfg


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fits(dev, tmp_path_factory):
    """case -> (config, trainer after 2 steps on grid_coords, checkpoint path, radii, data); each fit is made once"""
    from inr_mi355x.grid import GridSpec, grid_coords, grid_rows
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    made, folder = {}, tmp_path_factory.mktemp("ckpt")
    C, H, W = SHAPE

    def get(case):
        if case not in made:
            cfg = _config(case)
            image, _, shape = make_kspace(C, H, W, image_space=bool(cfg.get("transform", False)))
            coords = grid_coords(C, H, W, device=dev)
            if case == "MultiscaleKFourier":
                dist = grid_rows(GridSpec(C, H, W), 0, C * H * W, device=dev)[1]
                tr, radii = MultiscaleTrainer(cfg, image, coords, dist, RADII, shape, dev, seed=1), RADII
            else:
                tr, radii = INRTrainer(cfg, image, coords, shape, dev, seed=3), None
            tr.fit(2)
            path = str(folder / f"{case}.pt")
            torch.save(tr.checkpoint(), path)  # the file a training command writes
            made[case] = (cfg, tr, path, radii, image)
        return made[case]

    return get


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- per-model round trip ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["SIREN", "FFN", "WIRE", "WIRE2D", "Fourier", "Gabor", "KGabor", "MultiscaleKFourier",
                                  "SIREN_LogF"])
def test_round_trip_bit_equal_to_predict_all(dev, fits, case):
    from inr_mi355x.reconstruct import Reconstructor
    cfg, tr, path, radii, _ = fits(case)
    C, H, W = SHAPE
    rec = Reconstructor(cfg, path, shape=SHAPE, device=dev, radii=radii)
    assert rec.engine.exp_avg is None and rec.engine.exp_avg_sq is None and rec.engine.grads is None  # no Adam state
    assert not hasattr(rec, "image") and not hasattr(rec, "coords")  # no data
    want = tr.predict_all(chunk=300)
    got = rec.render(chunk=300)
    assert got.shape == (C, H, W, 2) and got.dtype == torch.float32 and got.device == dev
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert _bits_equal(got.reshape(-1, 2), want), float((got.reshape(-1, 2) - want).abs().max())
    # another chunking: the forward tolerance of tests/test_gpu_parity.py
    odd = rec.render(chunk=97).reshape(-1, 2)
    whole = tr.predict_all()
    record_parity(f"reconstruct/round_trip[{case}]", chunk97_abs_dev=float((odd - whole).abs().max()))
    torch.testing.assert_close(odd, whole, rtol=1e-5, atol=1e-6)
    # the checkpoint dict itself is accepted as well, and scoring goes through validate()'s kernel
    rec2 = Reconstructor(cfg, torch.load(path, map_location=dev), shape=SHAPE, device=dev, radii=radii)
    assert _bits_equal(rec2.render(chunk=300), got)


def test_compare_equals_trainer_metrics(dev, fits):
    from inr_mi355x.reconstruct import Reconstructor
    for case in ("SIREN", "SIREN_image"):
        cfg, tr, path, radii, image = fits(case)
        rec = Reconstructor(cfg, path, shape=SHAPE, device=dev)
        got = rec.compare(rec.render(), image)
        want = tr.metrics()
        assert got == want, (case, got, want)  # same prediction bits, same kernel
        with pytest.raises(ValueError, match="own grid"):
            rec.compare(rec.render(scale=2), image)


# ---- window, subset and resolution -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["SIREN", "KGabor", "MultiscaleKFourier"])
def test_window_subset_resolution_against_restated_coordinates(dev, fits, case):
    from inr_mi355x.grid import GridSpec, grid_rows_numpy
    from inr_mi355x.reconstruct import Reconstructor
    cfg, tr, path, radii, _ = fits(case)
    rec = Reconstructor(cfg, path, shape=SHAPE, device=dev, radii=radii)
    got = rec.render(height=31, width=45, window=WINDOW, coils=[1])
    assert got.shape == (1, 31, 45, 2)
    spec = GridSpec(SHAPE[0], 31, 45, coils=[1], window=WINDOW)
    coords, dist = (torch.from_numpy(a).to(dev) for a in grid_rows_numpy(spec, 0, spec.rows))
    if case == "SIREN":
        want = rec.engine.forward(coords, rec.enc_B, save=False)
    else:
        want = rec.engine.forward(coords, rec.enc_B, save=False, dist=dist)[-1]
    assert _bits_equal(got.reshape(-1, 2), want)
    # chunked, the rows are the same rows
    torch.testing.assert_close(rec.render(height=31, width=45, window=WINDOW, coils=[1], chunk=97), got, rtol=1e-5, atol=1e-6)
    # scale: rounded to the nearest integer, never below 1; height / width override it
    assert rec.render(scale=2).shape == (2, 48, 40, 2)
    assert rec.render(scale=0.01, coils=[1, 0, 1]).shape == (3, 1, 1, 2)
    assert rec.render(scale=2, height=5).shape == (2, 5, 40, 2)
    # a coil subset of the native grid is the matching slice of the native reconstruction
    native = rec.render()
    assert _bits_equal(rec.render(coils=[1])[0], native[1])


# ---- a trainer on the old host grid ------------------------------------------------------------------------------------
def test_trainer_on_create_coords_grid(dev):
    """The native reconstruction of a fit made on synthetic.create_coords' grid: the coordinates differ by at most
    2^-24, so the deviation from predict_all() is rounding-sized.  Bounded at 10 x the value first measured on the GPU
    (OLD_GRID_REL_DEV_MEASURED, relative to max|pred|): a wrong axis or a swapped window is ~1."""
    from inr_mi355x.reconstruct import Reconstructor
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    cfg = _config("SIREN")
    image, coords, shape = make_kspace(*SHAPE)
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    tr.fit(2)
    rec = Reconstructor(cfg, tr.checkpoint(), shape=SHAPE, device=dev)
    want = tr.predict_all()
    got = rec.render().reshape(-1, 2)
    rel = float((got - want).abs().max() / want.abs().max())
    swapped = rec.render(window=(1.0, -1.0, -1.0, 1.0)).reshape(-1, 2)  # what the bound must catch
    rel_swapped = float((swapped - want).abs().max() / want.abs().max())
    print(f"old grid: rel dev {rel:.3g} (bound {10 * OLD_GRID_REL_DEV_MEASURED:.3g}); flipped window: {rel_swapped:.3g}")
    record_parity("reconstruct/old_grid", rel_dev=rel, bound=10 * OLD_GRID_REL_DEV_MEASURED, rel_dev_flipped_window=rel_swapped)
    assert rel <= 10 * OLD_GRID_REL_DEV_MEASURED
    assert rel_swapped > 100 * OLD_GRID_REL_DEV_MEASURED


# ---- save() ------------------------------------------------------------------------------------------------------------
def _png_size(path):
    with open(path, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    w, h = struct.unpack(">II", head[16:24])
    return h, w


def test_save_writes_the_validation_epochs_files(dev, fits, tmp_path):
    from inr_mi355x import display as D
    from inr_mi355x.evalchain import ifft2c, image_metrics
    from inr_mi355x.reconstruct import Reconstructor
    cfg, tr, path, _, _ = fits("SIREN")
    rec = Reconstructor(cfg, path, shape=SHAPE, device=dev)
    pred = rec.render(height=31, width=45)
    out = tmp_path / "k"
    paths = rec.save(str(out), pred)
    assert [os.path.basename(p) for p in paths] == ["recon.npy", "recon.png", "recon_kspace.png"]
    assert all(os.path.exists(p) for p in paths)
    assert _png_size(paths[1]) == (31, 45) and _png_size(paths[2]) == (31, 45)
    rss = image_metrics(None, ifft2c(pred).contiguous())[0]
    assert _bits_equal(rec.rss(pred), rss)
    assert np.array_equal(D.read_png_gray(paths[1]), D.gray8(rss).cpu().numpy())
    assert np.array_equal(D.read_png_gray(paths[2]), D.gray8(D.kspace_display(pred)).cpu().numpy())
    back = np.load(paths[0])
    assert back.dtype == np.float32 and np.array_equal(back.view(np.int32), pred.cpu().numpy().view(np.int32))
    # an image-space config: no inverse FFT in front of the RSS, no k-space picture
    cfg_i, _, path_i, _, _ = fits("SIREN_image")
    rec_i = Reconstructor(cfg_i, path_i, shape=SHAPE, device=dev)
    pred_i = rec_i.render(scale=2)
    paths_i = rec_i.save(str(tmp_path / "i"), pred_i)
    assert [os.path.basename(p) for p in paths_i] == ["recon.npy", "recon.png"]
    assert not os.path.exists(tmp_path / "i" / "recon_kspace.png")
    assert _png_size(paths_i[1]) == (48, 40)
    rss_i = image_metrics(None, pred_i.contiguous())[0]
    assert np.array_equal(D.read_png_gray(paths_i[1]), D.gray8(rss_i).cpu().numpy())


# ---- other checks ------------------------------------------------------------------------------------------------------
def test_reference_written_checkpoint_renders(dev):
    from inr_mi355x.reconstruct import Reconstructor
    meta = json.load(open(os.path.join(GOLDEN, "trajectory_meta.json")))
    path = os.path.join(GOLDEN, "ref_checkpoint_SIREN_L2_step%d.pt" % meta["checkpoint_step"])
    shape = tuple(meta["shape"])
    rec = Reconstructor(meta["cases"]["SIREN_L2"], path, shape=shape, device=dev)
    ck = torch.load(path, map_location="cpu")
    for k, v in rec.model.state_dict().items():
        assert torch.equal(v.cpu(), ck["net"][k]), k
    assert torch.equal(rec.enc_B.cpu(), ck["enc"])
    pred = rec.render()
    assert pred.shape == (*shape, 2) and bool(torch.isfinite(pred).all()) and float(pred.abs().max()) > 0
    assert rec.render(scale=1.5, coils=[0]).shape == (1, int(shape[1] * 1.5 + 0.5), int(shape[2] * 1.5 + 0.5), 2)


def test_constructor_refusals(dev, fits):
    from inr_mi355x.reconstruct import Reconstructor
    cfg, _, path, radii, _ = fits("MultiscaleKFourier")
    with pytest.raises(ValueError, match="radii"):
        Reconstructor(cfg, path, shape=SHAPE, device=dev)
    with pytest.raises(ValueError, match="radii"):
        Reconstructor(dict(cfg, model="BoundedFourier"), path, shape=SHAPE, device=dev)
    cfg_s, _, path_s, _, _ = fits("SIREN")
    with pytest.raises(NotImplementedError, match="no MI355X kernel"):
        Reconstructor(dict(cfg_s, model="KAN"), path_s, shape=SHAPE, device=dev)
    with pytest.raises(ValueError, match="checkpoint"):
        Reconstructor(cfg_s, {"weights": 1}, shape=SHAPE, device=dev)


# ---- the command line --------------------------------------------------------------------------------------------------
def _cli(module, *args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, "-m", module, *args], cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_cli_train_then_reconstruct(dev, tmp_path):
    import yaml
    cfg = dict(_config("SIREN"), log_iter=1000, val_epoch=1, image_save_epoch=1000, normalization="coil")
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    fit_dir = tmp_path / "fit"
    trained = _cli("inr_mi355x.train", "--config", str(p), "--synthetic", "2,32,24", "--max_steps", "5",
                   "--output_path", str(fit_dir))
    ckpt = fit_dir / "model_000005.pt"
    assert trained["steps"] == 5 and ckpt.exists()
    base = ["--config", str(p), "--checkpoint", str(ckpt)]
    # native grid against the data
    r = _cli("inr_mi355x.reconstruct", *base, "--synthetic", "2,32,24", "--compare", "--output_path", str(tmp_path / "a"))
    assert r["shape"] == [2, 32, 24] and r["rows"] == 2 * 32 * 24 and r["seconds"] > 0 and r["rows_per_s"] > 0
    assert [os.path.basename(f) for f in r["files"]] == ["recon.npy", "recon.png", "recon_kspace.png"]
    gap = abs(r["psnr"] - trained["psnr"])
    print(f"cli: psnr train {trained['psnr']!r}, reconstruct {r['psnr']!r}, gap {gap:.3g} dB "
          f"(bound {10 * CLI_PSNR_GAP_DB_MEASURED:.3g})")
    record_parity("reconstruct/cli", psnr_train=trained["psnr"], psnr_reconstruct=r["psnr"], gap_db=gap,
                  bound=10 * CLI_PSNR_GAP_DB_MEASURED)
    assert gap <= 10 * CLI_PSNR_GAP_DB_MEASURED
    assert 0.0 < r["ssim"] <= 1.0
    # a finer grid, with no data at all
    r2 = _cli("inr_mi355x.reconstruct", *base, "--shape", "2,32,24", "--scale", "2", "--window", "-0.5,0.25,0.1,0.7",
              "--coils", "1", "--output_path", str(tmp_path / "b"))
    assert r2["shape"] == [1, 64, 48] and r2["rows"] == 64 * 48 and "psnr" not in r2
    assert _png_size(str(tmp_path / "b" / "recon.png")) == (64, 48)
    assert _png_size(str(tmp_path / "b" / "recon_kspace.png")) == (64, 48)
    assert np.load(tmp_path / "b" / "recon.npy").shape == (1, 64, 48, 2)
