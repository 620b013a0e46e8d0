"""Coil compression on the MI355X (``-m gpu``): inr_coil_gram and inr_coil_apply against the numpy definitions of
inr_mi355x/coils.py over every path of the kernels (one pixel, a tile less / exactly / more than one, several tiles with a
ragged end, odd N = the 8-byte path, 1 .. 32 coils = one pair with 256 slices .. 528 pairs on 256 lanes), the projector
of the device Gram matrix, a fit on virtual coils end to end, and the switch left off.

Criteria: Gram -- |dG_ij| <= 2 N 2^-53 sqrt(G_ii G_jj), the reordering bound of an fp64 sum of exact
products (sum |terms| <= sqrt(G_ii G_jj) by Cauchy-Schwarz); apply -- per component |d| <= 4 K 2^-24 sum_k |A_mk| |x_k[p]|,
the fp32 dot-product bound (4: two real products per complex term, and FMA contraction)."""
import argparse

import numpy as np
import pytest
import torch

from conftest import record_parity
from inr_mi355x import _lib as L
from inr_mi355x import coils as CC

pytestmark = pytest.mark.gpu

T = L.COIL_TILE_PIXELS
PIXELS = [1, T - 1, T, T + 1, 3 * T + 5, 33 * 31]  # the last one is passed as H x W = 33 x 31 (odd N)
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _scan(C, N, seed):
    """complex64 [C, N] whose magnitudes span six decades"""
    g = np.random.default_rng(seed)
    mag = 10.0 ** g.uniform(-3.0, 3.0, (C, N))
    return (mag * (g.standard_normal((C, N)) + 1j * g.standard_normal((C, N)))).astype(np.complex64)


def _pairs(z):
    return torch.from_numpy(np.stack([z.real, z.imag], -1).astype(np.float32))


@pytest.mark.parametrize("C", [1, 2, 15, 32])
def test_gram_matches_numpy(dev, C):
    for N in PIXELS:
        x = _scan(C, N, seed=100 * C + N % 97)
        shape = (C, 33, 31) if N == 33 * 31 else (C, N)
        data = _pairs(x).reshape(*shape, 2).to(dev)
        G = CC.coil_gram(data, shape)
        ref = CC.coil_gram_numpy(x)
        d = np.sqrt(np.outer(ref.diagonal().real, ref.diagonal().real))
        bound = 2.0 * N * 2.0 ** -53 * d
        err_re, err_im = np.abs(G.real - ref.real), np.abs(G.imag - ref.imag)
        record_parity("coil_gram", C=C, N=N, worst=float(np.max(np.maximum(err_re, err_im) / d)), bound=2.0 * N * 2.0 ** -53)
        assert np.all(err_re <= bound) and np.all(err_im <= bound), (C, N)
        assert np.array_equal(G, G.conj().T) and np.all(G.diagonal().imag == 0), (C, N)  # exactly Hermitian
        assert np.array_equal(G.real, G.real.T) and np.array_equal(G.imag, -G.imag.T)
        again = CC.coil_gram(data, shape)
        assert G.tobytes() == again.tobytes(), (C, N)  # fixed order: the same bits


def test_gram_unaligned_base_takes_the_8_byte_path(dev):
    """an even N whose base is only 8-byte aligned (a view one pixel into a buffer)"""
    C, N = 3, 2 * T + 6
    x = _scan(C, N, seed=7)
    buf = torch.zeros(C * N + 1, 2, device=dev)
    buf[1:] = _pairs(x).reshape(-1, 2).to(dev)
    view = buf[1:]
    assert view.data_ptr() % 16 == 8
    G, ref = CC.coil_gram(view, (C, N)), CC.coil_gram_numpy(x)
    d = np.sqrt(np.outer(ref.diagonal().real, ref.diagonal().real))
    assert np.all(np.abs(G - ref) <= 2.0 * np.sqrt(2.0) * N * 2.0 ** -53 * d)
    assert G.tobytes() == CC.coil_gram(_pairs(x).to(dev), (C, N)).tobytes()  # the two load paths add in the same order


@pytest.mark.parametrize("M,K", [(1, 1), (3, 6), (8, 15), (15, 8), (32, 32)])
def test_apply_matches_numpy_and_stays_in_bounds(dev, M, K):
    lib = L.load()
    g = np.random.default_rng(10 * M + K)
    A = ((g.standard_normal((M, K)) + 1j * g.standard_normal((M, K))) / np.sqrt(K)).astype(np.complex64)
    a_dev = _pairs(A).to(dev)
    for N in PIXELS:
        x = _scan(K, N, seed=1000 * M + K + N % 89)
        ref = CC.coil_apply_numpy(A, x)
        bound = 4.0 * K * 2.0 ** -24 * (np.abs(A).astype(np.float64) @ np.abs(x).astype(np.float64))
        got = CC.coil_apply(_pairs(x).to(dev), A, (K, N)).cpu().numpy()
        assert got.shape == (M, N, 2)
        err = np.maximum(np.abs(got[..., 0] - ref.real), np.abs(got[..., 1] - ref.imag))
        record_parity("coil_apply", M=M, K=K, N=N, worst=float(np.max(err / bound)))
        assert np.all(err <= bound), (M, K, N)
        # guard words before and after out, through the ABI itself
        buf = torch.full((GUARD + M * N * 2 + GUARD,), 12345.0, device=dev)
        out = buf[GUARD:GUARD + M * N * 2]
        xin = _pairs(x).to(dev).contiguous()
        L.check(lib.inr_coil_apply(xin.data_ptr(), a_dev.data_ptr(), M, K, N, out.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream))
        host = buf.cpu().numpy()
        assert np.all(host[:GUARD] == 12345.0) and np.all(host[GUARD + M * N * 2:] == 12345.0), (M, K, N)
        assert np.array_equal(host[GUARD:GUARD + M * N * 2].reshape(M, N, 2), got), (M, K, N)


def test_apply_refuses_overlap_on_the_device(dev):
    lib = L.load()
    x = torch.zeros(4, 100, 2, device=dev)
    a = torch.zeros(4, 4, 2, device=dev)
    assert lib.inr_coil_apply(x.data_ptr(), a.data_ptr(), 4, 4, 100, x.data_ptr(), None) == -1
    assert "overlaps" in L.last_error()


@pytest.fixture(scope="module")
def synthetic15():
    from inr_mi355x.synthetic import make_kspace
    image, _, shape = make_kspace(15, 64, 48, normalization=None)
    return image.reshape(*shape, 2)


@pytest.mark.parametrize("K", [5, 7])
def test_projector_of_the_device_gram(dev, synthetic15, K):
    """K sits at a clear gap of the spectrum; the rows may differ by more than the projector does"""
    G_dev = CC.coil_gram(synthetic15.to(dev), (15,))
    G_ref = CC.coil_gram_numpy(synthetic15)
    w = np.linalg.eigvalsh(G_ref)[::-1]
    assert w[K - 1] / w[K] > 5
    A = CC.compression_matrix(G_dev, K, dtype=np.complex128)[0]
    B = CC.compression_matrix(G_ref, K, dtype=np.complex128)[0]
    diff = np.linalg.norm(A.conj().T @ A - B.conj().T @ B)
    record_parity("coil_projector", K=K, diff=float(diff), gap=float(w[K - 1] / w[K]))
    assert diff <= 1e-9


def test_compress_on_the_device_matches_numpy(dev, synthetic15):
    virtual, rec = CC.compress(synthetic15.to(dev), 8)
    ref_v, ref = CC.compress_numpy(synthetic15, 8)
    assert virtual.shape == (8, 64, 48, 2) and rec.coils_in == 15 and rec.coils_out == 8
    assert rec.energy_kept == pytest.approx(ref.energy_kept, rel=1e-12) and rec.energy_kept > 0.9999
    assert rec.rss_psnr > 60 and abs(rec.rss_psnr - ref.rss_psnr) < 0.05  # fp32 rounding of y against a 4e-4 error
    back = rec.expand(virtual)
    assert back.shape == (15, 64, 48, 2)
    x = CC._as_complex(synthetic15.numpy()).reshape(15, -1)
    y = CC._as_complex(virtual.cpu().numpy()).reshape(8, -1)
    AH = rec.matrix.conj().T
    want = CC.coil_apply_numpy(AH, y)
    bound = 4.0 * 8 * 2.0 ** -24 * (np.abs(AH).astype(np.float64) @ np.abs(y).astype(np.float64))
    got = CC._as_complex(back.cpu().numpy()).reshape(15, -1)
    assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)
    # the projection keeps the scan up to the energy dropped
    lost = np.linalg.norm(got - x) ** 2 / np.linalg.norm(x) ** 2
    assert lost <= (1 - rec.energy_kept) * 1.01 + 1e-6


CFG = dict(loss="L2", lr=1e-3, batch_size=300, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999, model="SIREN",
           encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
           net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32))


def test_fit_on_virtual_coils_end_to_end(dev, tmp_path):
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.reconstruct import Reconstructor
    from inr_mi355x.train import INRTrainer
    opts = argparse.Namespace(synthetic="6,16,12")
    cfg = dict(CFG, virtual_coils=3)
    image, coords, shape, cc = cli_fit_data(opts, cfg, "coil")
    assert shape == (3, 16, 12) and image.shape == (3 * 16 * 12, 2) and coords.shape == (3 * 16 * 12, 3)
    assert cc.coils_in == 6 and cc.coils_out == 3 and cc.matrix.shape == (3, 6) and 0 < cc.energy_kept <= 1
    # normalised AFTER compression: 'coil' leaves every virtual coil with max |.| = 1
    mags = image.reshape(3, -1, 2).pow(2).sum(-1).sqrt().max(dim=1)[0].cpu().numpy()
    assert np.allclose(mags, 1.0, rtol=1e-6)
    tr = INRTrainer(cfg, image, grid_coords(3, 16, 12, device=dev), shape, dev, seed=3, coil_compression=cc)
    assert tuple(tr.shape) == (3, 16, 12)
    tr.fit(4)
    assert tr.global_step == 4
    rec = tr.validate(0)
    assert rec["coil_compression"] == cc.summary() == {"coils_in": 6, "coils_out": 3, "energy_kept": cc.energy_kept,
                                                       "rss_psnr": cc.rss_psnr}
    assert tr.metrics()["coil_compression"] == cc.summary()
    ckpt = tr.checkpoint()
    assert set(ckpt) == {"net", "enc", "opt", "coil_compression"}
    st = ckpt["coil_compression"]
    assert np.array_equal(st["matrix"].numpy(), cc.matrix) and st["coils_in"] == 6 and st["coils_out"] == 3
    assert np.array_equal(st["eigenvalues"].numpy(), cc.eigenvalues)
    path = str(tmp_path / "model.pt")
    torch.save(ckpt, path)

    r = Reconstructor(cfg, path, shape, dev)
    pred = r.render()
    assert pred.shape == (3, 16, 12, 2) and torch.equal(pred.reshape(-1, 2), tr.predict_all())
    phys = r.expand(pred)
    assert phys.shape == (6, 16, 12, 2)
    want = cc.expand_numpy(pred.cpu().numpy())
    assert np.allclose(CC._as_complex(phys.cpu().numpy()).reshape(6, -1), want, rtol=1e-4, atol=1e-6)
    # compare() with the scan through the STORED matrix is the trainer's own evaluate(): 1e-4 dB covers the fp32
    # reductions of the two PSNR implementations over 192 pixels (relative 2.3e-5 of the mean squared error)
    again = cli_fit_data(opts, dict(CFG), "coil", matrix=r.coil_compression)
    assert again[2] == shape and torch.equal(again[0], image)
    assert abs(r.compare(pred, again[0])["psnr"] - tr.evaluate()) < 1e-4
    with pytest.raises(ValueError, match="3 virtual coils.*C = 6"):
        Reconstructor(cfg, path, (6, 16, 12), dev)

    # a checkpoint without compression is refused by this trainer, and the other way round
    plain_data = cli_fit_data(opts, dict(CFG), "coil")
    assert plain_data[3] is None and plain_data[2] == (6, 16, 12)
    plain = INRTrainer(dict(CFG), *plain_data[:3], dev, seed=3)
    assert "coil_compression" not in plain.checkpoint() and set(plain.checkpoint()) == {"net", "enc", "opt"}
    with pytest.raises(ValueError, match="coil compression"):
        tr.load_checkpoint(plain.checkpoint())
    with pytest.raises(ValueError, match="coil compression"):
        plain.load_checkpoint(ckpt)
    with pytest.raises(ValueError, match="coil compression"):
        tr.load_checkpoint(dict(ckpt, coil_compression=dict(st, coils_in=8)))
    tr.load_checkpoint(ckpt)
    with pytest.raises(ValueError, match="virtual_coils"):
        INRTrainer(dict(CFG, virtual_coils=7), *plain_data[:3], dev, seed=3)


def test_switch_off_is_bit_identical(dev):
    from inr_mi355x.cli import cli_fit_data
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    want = make_kspace(6, 16, 12, normalization="coil")
    got = cli_fit_data(argparse.Namespace(synthetic="6,16,12"), dict(CFG), "coil")
    tr = INRTrainer(dict(CFG), *got[:3], dev, seed=3)
    assert tr.coil_compression is None and tuple(tr.shape) == (6, 16, 12)
    assert tr.image.cpu().numpy().tobytes() == want[0].numpy().tobytes()
    assert tr.coords.cpu().numpy().tobytes() == want[1].numpy().tobytes()
    tr.fit(1)
    assert "coil_compression" not in tr.validate(0) and "coil_compression" not in tr.metrics()
