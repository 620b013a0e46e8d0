"""Coil compression on the host (inr_mi355x/coils.py): the numpy definitions the kernels are held
to -- compression matrix, RSS invariance, exact low rank, the synthetic scan -- the refusals, the header's declarations,
the library's argument checks on fake pointers, and the switch left off.  None of it touches a GPU."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import coils as CC
from inr_mi355x.synthetic import make_kspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24


def _random_scan(C, N, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal((C, N)) + 1j * g.standard_normal((C, N))).astype(np.complex64)


def _dot_bound(A, x):
    """per component: 4 K 2^-24 sum_k |A_mk| |x_k[p]| (the fp32 dot-product bound of DESIGN 4.18)"""
    return 4.0 * A.shape[1] * U24 * (np.abs(A).astype(np.float64) @ np.abs(x).astype(np.float64))


@pytest.fixture(scope="module")
def scan():
    image, _, shape = make_kspace(15, 64, 48, normalization=None)
    return image.reshape(*shape, 2)


def test_compression_matrix_orthonormal_ordered_and_phased():
    x = _random_scan(7, 300, seed=1) * np.linspace(1.0, 3.0, 7)[:, None].astype(np.float32)
    G = CC.coil_gram_numpy(x)
    assert G.dtype == np.complex128 and np.array_equal(G, G.conj().T)
    assert np.allclose(G, x.astype(np.complex128) @ x.astype(np.complex128).conj().T, rtol=1e-13, atol=0)
    for K in (1, 4, 7):
        A, w, kept = CC.compression_matrix(G, K)
        assert A.dtype == np.complex64 and A.shape == (K, 7) and w.dtype == np.float64 and w.shape == (7,)
        A64 = CC.compression_matrix(G, K, dtype=np.complex128)[0]
        assert A64.dtype == np.complex128 and np.array_equal(A64.astype(np.complex64), A)
        w_ref, V = np.linalg.eigh(G)
        assert np.array_equal(w, w_ref[::-1]) and np.all(np.diff(w) <= 0)
        # A A^H = I to 1e-12 in float64, before the cast (the complex64 cast alone costs 2^-24 per entry)
        rows = V[:, ::-1][:, :K].conj().T
        assert np.abs(A64 @ A64.conj().T - np.eye(K)).max() <= 1e-12
        A32 = A.astype(np.complex128)
        assert np.abs(A32 @ A32.conj().T - np.eye(K)).max() <= 8 * 7 * U24
        for m in range(K):
            k = int(np.argmax(np.abs(A[m])))
            assert A[m, k].imag == 0 and A[m, k].real > 0
            # the row is its eigenvector, conjugated, times a unit complex number
            ratio = A64[m] / rows[m]
            assert np.abs(np.abs(ratio) - 1).max() < 1e-6 and np.abs(ratio - ratio[0]).max() < 1e-5
        assert kept == pytest.approx(w[:K].sum() / w.sum(), rel=1e-14)
    assert CC.compression_matrix(G, 7)[2] == pytest.approx(1.0, abs=1e-14)


def test_rss_is_invariant_with_all_coils_kept():
    x = _random_scan(6, 257, seed=2)
    A, _, _ = CC.compression_matrix(CC.coil_gram_numpy(x), 6)
    y = CC.coil_apply_numpy(A, x)
    assert y.dtype == np.complex64 and y.shape == x.shape
    ss_x = (np.abs(x.astype(np.complex128)) ** 2).sum(0)
    ss_y = (np.abs(y.astype(np.complex128)) ** 2).sum(0)
    # |y|^2 - |x|^2 <= 2 |y| dy with dy the dot-product bound, plus A's own distance from unitary after the cast
    dy = np.sqrt(2.0) * _dot_bound(A, x)
    bound = (2 * np.abs(y) * dy + dy ** 2).sum(0) + 4 * 6 * U24 * ss_x
    assert np.all(np.abs(ss_y - ss_x) <= bound)


def test_exact_low_rank_is_recovered():
    g = np.random.default_rng(3)
    src = g.standard_normal((3, 500)) + 1j * g.standard_normal((3, 500))
    mix = g.standard_normal((7, 3)) + 1j * g.standard_normal((7, 3))
    x = (mix @ src).astype(np.complex64)
    # (the fp32 cast of the mixture leaves rank-7 rounding noise of relative energy ~ 2^-48)
    pairs = np.stack([x.real, x.imag], -1).reshape(7, 25, 20, 2)
    virtual, rec = CC.compress_numpy(pairs, 3)
    assert rec.energy_kept >= 1 - 1e-10 and rec.coils_in == 7 and rec.coils_out == 3
    assert virtual.shape == (3, 25, 20, 2) and virtual.dtype == np.float32
    back = rec.expand_numpy(virtual)
    A = rec.matrix
    y = CC.coil_apply_numpy(A, x)
    # two chained products: the second one's bound, plus the first one's error carried through |A^H|, plus the
    # complex64 cast of A (A^H A x against x on the retained subspace: <= 2^-23 per entry of A, twice)
    AH = A.conj().T
    bound = np.sqrt(2.0) * (_dot_bound(AH, y) + np.abs(AH).astype(np.float64) @ _dot_bound(A, x)) \
        + 4 * U24 * (np.abs(AH).astype(np.float64) @ (np.abs(A).astype(np.float64) @ np.abs(x)))
    assert np.all(np.abs(back - x) <= bound)
    assert np.abs(back - x).max() < 1e-4 * np.abs(x).max()


def test_synthetic_scan_compresses(scan):
    virtual, rec = CC.compress_numpy(scan, 8)
    print("synthetic 15x64x48 -> 8: energy_kept %.7f, rss_psnr %.2f dB" % (rec.energy_kept, rec.rss_psnr))
    assert virtual.shape == (8, 64, 48, 2)
    assert rec.energy_kept > 0.9999 and rec.rss_psnr > 60
    assert rec.summary() == {"coils_in": 15, "coils_out": 8, "energy_kept": rec.energy_kept, "rss_psnr": rec.rss_psnr}
    st = rec.state()
    back = CC.CoilCompression.from_state(st)
    assert np.array_equal(back.matrix, rec.matrix) and np.array_equal(back.eigenvalues, rec.eigenvalues)
    assert CC.same_compression(st, st) is None and CC.same_compression(None, None) is None
    assert CC.same_compression(st, None) and CC.same_compression(None, st)
    assert CC.same_compression(st, dict(st, coils_out=7))


def test_refusals(scan):
    G = CC.coil_gram_numpy(_random_scan(4, 10))
    for bad in (5, -1, 2.5, "3", True):
        with pytest.raises(ValueError):
            CC.compression_matrix(G, bad)
        with pytest.raises(ValueError):
            CC.check_virtual_coils(bad, 4)
    with pytest.raises(ValueError, match="32"):
        CC.check_virtual_coils(3, 33)
    assert CC.check_virtual_coils(None, 4) == 0 and CC.check_virtual_coils(0, 33) == 0 and CC.check_virtual_coils(4, 4) == 4
    with pytest.raises(ValueError):
        CC.compress_numpy(np.zeros((33, 2, 2, 2), np.float32), 3)
    # a CPU tensor never falls back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.coil_gram(scan, (15,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.coil_apply(scan, np.eye(15, dtype=np.complex64), (15,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.compress(scan, 8)


def test_trainer_refuses_bad_switch_before_any_launch():
    """config['virtual_coils'] is checked by ResidentFit._init_fit, the first call of every trainer's constructor"""
    from inr_mi355x.trainer_base import ResidentFit
    rec = CC.CoilCompression(np.eye(3, 6, dtype=np.complex64), np.ones(6), 6, 3, 1.0, 99.0)
    for cfg, shape, cc in (({"virtual_coils": -1}, (6, 4, 4), None), ({"virtual_coils": 2.5}, (6, 4, 4), None),
                           ({"virtual_coils": 7}, (6, 4, 4), None),  # K > C: the data cannot have come through it
                           ({"virtual_coils": 3}, (6, 4, 4), None), ({"virtual_coils": 3}, (6, 4, 4), rec),
                           ({"virtual_coils": 4}, (3, 4, 4), rec), ({}, (3, 4, 4), rec)):
        with pytest.raises(ValueError, match="virtual_coils"):
            ResidentFit()._init_fit(cfg, shape, "cpu", 0, 0, 1, None, coil_compression=cc)
    fit = ResidentFit()
    fit._init_fit({"virtual_coils": 3}, (3, 4, 4), "cpu", 0, 0, 1, None, coil_compression=rec)
    assert fit.coil_compression is rec
    fit._init_fit({}, (6, 4, 4), "cpu", 0, 0, 1, None)
    assert fit.coil_compression is None and fit.config["virtual_coils"] == 0


def test_header_declares_the_three_entries():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^int (inr_coil_(?:gram|apply)\w*)\(", text, re.M))
    assert declared == {"inr_coil_gram", "inr_coil_gram_scratch", "inr_coil_apply"}
    assert re.search(r"^int inr_coil_gram_scratch\(int32_t C, int64_t N, int64_t\* scratch_doubles\);", text, re.M)
    macros = dict(re.findall(r"^#define (INR_COIL_\w+) (\d+)", text, re.M))
    assert int(macros["INR_COIL_MAX"]) == L.COIL_MAX == 32
    assert int(macros["INR_COIL_TILE_PIXELS"]) == L.COIL_TILE_PIXELS
    assert int(re.search(r"^#define INR_ABI_VERSION (\d+)", text, re.M).group(1)) == L.ABI_VERSION == 7
    lib = L.load()
    for name in declared:
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.inr_abi_version() == 7


def test_argument_checks_need_no_gpu():
    lib = L.load()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30)
    n = ctypes.c_int64(-1)
    assert lib.inr_coil_gram_scratch(15, 1000, ctypes.byref(n)) == 0 and n.value > 0
    need = n.value
    m = ctypes.c_int64(-1)
    assert lib.inr_coil_gram_scratch(15, 1000, ctypes.byref(m)) == 0 and m.value == need  # a pure function
    assert need % (2 * 15 * 16 // 2) == 0  # blocks x pairs x (re, im)
    assert CC.scratch_doubles(15, 1000) == need
    for C_ in (0, 33):
        assert lib.inr_coil_gram_scratch(C_, 1000, ctypes.byref(n)) == -1 and "1..32" in L.last_error()
        assert lib.inr_coil_gram(fake, C_, 1000, other, other, 1 << 40, None) == -1 and "1..32" in L.last_error()
    assert lib.inr_coil_gram_scratch(15, 0, ctypes.byref(n)) == -1
    assert lib.inr_coil_gram(None, 15, 1000, other, other, need, None) == -1 and "null" in L.last_error()
    assert lib.inr_coil_gram(fake, 15, 1000, other, other, need - 1, None) == -1 and "scratch" in L.last_error()
    assert lib.inr_coil_gram(ctypes.c_void_p(4100), 15, 1000, other, other, need, None) == -1 and "aligned" in L.last_error()
    for M, K in ((0, 4), (33, 4), (4, 0), (4, 33)):
        assert lib.inr_coil_apply(fake, other, M, K, 1000, ctypes.c_void_p(1 << 31), None) == -1 and "1..32" in L.last_error()
    assert lib.inr_coil_apply(fake, other, 4, 4, 0, ctypes.c_void_p(1 << 31), None) == -1
    assert lib.inr_coil_apply(fake, None, 4, 4, 1000, ctypes.c_void_p(1 << 31), None) == -1 and "null" in L.last_error()
    assert lib.inr_coil_apply(fake, other, 4, 4, 1000, fake, None) == -1 and "overlaps" in L.last_error()  # out == in
    assert lib.inr_coil_apply(fake, other, 8, 4, 1000, ctypes.c_void_p(4096 + 4 * 1000 * 8 - 8), None) == -1  # last pixel
    assert "overlaps" in L.last_error()
    assert lib.inr_coil_apply(fake, other, 4, 4, 1000, ctypes.c_void_p((1 << 30) + 8), None) == -1 and "A" in L.last_error()


def test_switch_off_is_todays_path(tmp_path):
    from inr_mi355x.cli import cli_data, cli_fit_data, parse_cli
    from inr_mi355x.hp_search import DATA_KEYS
    from inr_mi355x.trainer_base import set_default_configs
    assert set_default_configs({})["virtual_coils"] == 0 and "virtual_coils" in DATA_KEYS
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model: SIREN\nnormalization: max\n")
    opts, config = parse_cli(argv=["--config", str(cfg), "--synthetic", "3,12,10"])
    assert opts.virtual_coils is None and config["virtual_coils"] == 0
    want = make_kspace(3, 12, 10, normalization="max")
    for got in (cli_data(opts, config, "coil"), cli_fit_data(opts, config, "coil")):
        assert got[0].numpy().tobytes() == want[0].numpy().tobytes() and got[1].numpy().tobytes() == want[1].numpy().tobytes()
        assert got[2] == want[2] and not got[0].is_cuda
    assert cli_fit_data(opts, config, "coil")[3] is None and len(cli_data(opts, config, "coil")) == 3
    want = make_kspace(3, 12, 10, normalization="coil", image_space=True)
    got = cli_data(opts, {"virtual_coils": 0}, "coil", image_space=True)
    assert got[0].numpy().tobytes() == want[0].numpy().tobytes()
    opts, config = parse_cli(argv=["--config", str(cfg), "--virtual-coils", "2"])
    assert config["virtual_coils"] == 2
    with pytest.raises(ValueError):  # K > C is refused before anything is generated or launched
        cli_fit_data(argparse.Namespace(synthetic="3,12,10"), {"virtual_coils": 4}, "coil")
    from inr_mi355x import reconstruct
    r = reconstruct.parse_args(["--config", str(cfg), "--checkpoint", "x.pt", "--shape", "2,8,8", "--expand-coils"])
    assert r.expand_coils
    with pytest.raises(SystemExit):
        reconstruct.parse_args(["--config", str(cfg), "--checkpoint", "x.pt", "--shape", "2,8,8", "--expand-coils",
                                "--coils", "0"])
