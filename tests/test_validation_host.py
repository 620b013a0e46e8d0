"""Host-side checks of the validation epoch: a float64 restatement of scikit-image 0.18.1's SSIM (the GPU tests'
yardstick; scikit-image itself is not available), the reference's bookkeeping quirks, and the C-ABI surface of the
image-metrics kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def box7(a: np.ndarray) -> np.ndarray:
    """7 x 7 window sums of the fully-inside windows: [H-6, W-6], entry (i, j) = sum of a[i:i+7, j:j+7]."""
    return np.lib.stride_tricks.sliding_window_view(a, (7, 7)).sum(axis=(-2, -1))


def ssim64(x, xhat) -> float:
    """skimage.metrics.structural_similarity(x, xhat, data_range=R) of scikit-image 0.18.1 as models/utils.py:227-233
    calls it: R = max(x.max, xhat.max) - min(x.min, xhat.min) in float32; images cast to float64; 7 x 7 uniform window,
    K1 = 0.01, K2 = 0.03, sample covariance; the mean over the interior cropped by 3 pixels, where every window lies
    inside the image (so the filter's boundary mode does not matter)."""
    x = np.asarray(x, dtype=np.float32)
    xhat = np.asarray(xhat, dtype=np.float32)
    if min(x.shape) < 7:
        raise ValueError("win_size exceeds image extent")
    R = np.float64(np.maximum(x.max(), xhat.max()) - np.minimum(x.min(), xhat.min()))
    X, Y = x.astype(np.float64), xhat.astype(np.float64)
    NP = 49
    ux, uy = box7(X) / NP, box7(Y) / NP
    uxx, uyy, uxy = box7(X * X) / NP, box7(Y * Y) / NP, box7(X * Y) / NP
    cov = NP / (NP - 1)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    with np.errstate(invalid="ignore"):
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        return float(S.mean())


def ssim_scipy(x, xhat) -> float:
    """The same statistic written the way scikit-image 0.18.1 writes it, on scipy.ndimage.uniform_filter."""
    nd = pytest.importorskip("scipy.ndimage")
    x = np.asarray(x, dtype=np.float32)
    xhat = np.asarray(xhat, dtype=np.float32)
    R = np.maximum(x.max(), xhat.max()) - np.minimum(x.min(), xhat.min())
    # (K1 * R) ** 2 with R a float32 scalar is float64 under the numpy 1.x the reference pins (scalar-scalar promotion);
    # numpy >= 2 would keep it in float32
    R = np.float64(R)
    X, Y = x.astype(np.float64), xhat.astype(np.float64)
    f = lambda a: nd.uniform_filter(a, size=7)  # noqa: E731
    ux, uy = f(X), f(Y)
    uxx, uyy, uxy = f(X * X), f(Y * Y), f(X * Y)
    cov = 49 / 48
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    with np.errstate(invalid="ignore"):
        S = (A1 * A2) / (B1 * B2)
        return float(S[3:-3, 3:-3].mean())


@pytest.mark.parametrize("case", ["random", "smooth", "constant", "tiny", "identical"])
def test_ssim_restatement_matches_uniform_filter_form(case):
    rng = np.random.default_rng(7)
    if case == "random":
        x, y = rng.random((64, 45)), rng.random((64, 45))
    elif case == "smooth":
        yy, xx = np.meshgrid(np.linspace(-1, 1, 40), np.linspace(-1, 1, 33), indexing="ij")
        x = np.exp(-(xx ** 2 + yy ** 2) * 3)
        y = x + 0.01 * rng.standard_normal(x.shape)
    elif case == "constant":
        x, y = np.full((20, 17), 0.25), rng.random((20, 17))
    elif case == "tiny":
        x, y = rng.random((7, 7)), rng.random((7, 7))
    else:
        x = rng.random((30, 31))
        y = x.copy()
    a, b = ssim64(x, y), ssim_scipy(x, y)
    assert abs(a - b) <= 1e-12, (a, b)
    if case == "identical":
        assert abs(a - 1.0) <= 1e-12


def test_ssim_restatement_edge_cases():
    with pytest.raises(ValueError):
        ssim64(np.zeros((6, 40)), np.zeros((6, 40)))
    assert np.isnan(ssim64(np.full((9, 9), 0.5), np.full((9, 9), 0.5)))  # R = 0: 0 / 0, as skimage


def _tracker():
    from inr_mi355x.validation import ValidationMixin

    class T(ValidationMixin):
        pass
    t = T()
    t._init_validation()
    return t


def test_best_epoch_bookkeeping_is_strict_and_zero_based():
    """train.py:146-149,232-237: initial -999999 / -1, strict '>', the stored epoch is the loop's 0-based epoch."""
    t = _tracker()
    assert (t.best_psnr, t.best_psnr_ep, t.best_ssim, t.best_ssim_ep) == (-999999, 0, -1, 0)
    t.update_best(0, 20.0, 0.5)
    t.update_best(1, 20.0, 0.6)   # equal PSNR does not move the record
    t.update_best(2, 19.0, 0.6)   # equal SSIM does not either
    t.update_best(3, 21.5, float("nan"))  # NaN never wins
    assert (t.best_psnr, t.best_psnr_ep) == (21.5, 3)
    assert (t.best_ssim, t.best_ssim_ep) == (0.6, 1)


def test_test_loss_is_divided_by_the_train_loader_length():
    """train.py:242: the summed val-batch loss over len(data_loader) -- the TRAIN loader."""
    t = _tracker()
    m = torch.tensor([30.0, 0.75], dtype=torch.float64)
    rec = t._finish_validation(4, m, torch.tensor(6.0, dtype=torch.float64), n_train_batches=4)
    assert rec == {"epoch": 4, "test_loss": 1.5, "psnr": 30.0, "ssim": 0.75}
    rec = t._finish_validation(5, m, None, n_train_batches=4)
    assert rec["test_loss"] is None and len(t.val_history) == 2


def test_validation_line_is_the_references():
    t = _tracker()
    rec = t._finish_validation(1, torch.tensor([31.23456, 0.876543], dtype=torch.float64),
                               torch.tensor(0.5, dtype=torch.float64), 2)
    assert t.validation_line(rec, 10) == ("[Validation Epoch: 2/10] Test loss: 0.25 | Test psnr: 31.23 | Test ssim: 0.8765 "
                                          "\n Best psnr: 31.23 @ epoch 1 | Best ssim: 0.8765 @ epoch 1")


def _last_head_only(outs, gt, scale):
    """train_kspace_multiscale.py:214-224 as written: test_loss is REASSIGNED per head."""
    test_loss = 0
    for out in outs:
        test_loss = scale * torch.mean((out - gt) ** 2)
    return test_loss


def test_multiscale_test_loss_is_the_last_heads():
    """The quirk validate() reproduces: only the last head's loss survives the loop, not the sum over heads."""
    g = torch.Generator().manual_seed(0)
    outs = [torch.randn(50, 2, generator=g) for _ in range(4)]
    gt = torch.randn(50, 2, generator=g)
    got = _last_head_only(outs, gt, 0.5)
    assert torch.equal(got, 0.5 * torch.mean((outs[-1] - gt) ** 2))
    assert not torch.allclose(got, sum(0.5 * torch.mean((o - gt) ** 2) for o in outs))
    import inspect
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    src = inspect.getsource(MultiscaleTrainer.validate)
    assert "pred = self.predict_all()" in src  # predict_all returns outs[-1] (the last head) only


def test_image_metrics_in_header_symbols_and_library():
    """include/inr_abi.h declares inr_image_metrics*, _lib.SYMBOLS binds them and the built .so exports them."""
    from inr_mi355x import _lib
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\bint\s+(inr_image_metrics\w*)\s*\(", hdr))
    assert declared == {"inr_image_metrics", "inr_image_metrics_scratch"}
    assert declared <= set(_lib.SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert re.search(r"v7 additions", hdr) and "#define INR_ABI_VERSION 7" in hdr


def test_image_metrics_scratch_query_and_argument_checks():
    """The sizing query and the argument checks run on the host (no GPU needed): a short scratch and H < 7 are
    refused with the library's message before anything is launched."""
    from inr_mi355x import _lib as L
    lib = L.load()
    n = ctypes.c_int64()
    L.check(lib.inr_image_metrics_scratch(15, 640, 368, ctypes.byref(n)))
    assert n.value >= 5 * 1 + 1
    assert lib.inr_image_metrics_scratch(0, 640, 368, ctypes.byref(n)) != 0
    fake = ctypes.c_void_p(16)  # never dereferenced: the call fails its checks first
    rc = lib.inr_image_metrics(fake, 2, 6, 40, fake, fake, fake, fake, 10 ** 6, None)
    assert rc != 0 and "win_size exceeds image extent" in L.last_error()
    rc = lib.inr_image_metrics(fake, 2, 64, 40, fake, fake, fake, fake, 1, None)
    assert rc != 0 and "scratch" in L.last_error()


def test_evalchain_metrics_refuse_cpu_tensors():
    from inr_mi355x import evalchain as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.image_metrics(torch.rand(9, 9), torch.rand(1, 9, 9, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ssim(torch.rand(9, 9), torch.rand(9, 9))
