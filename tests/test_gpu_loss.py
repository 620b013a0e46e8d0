"""The loss family (``loss_row`` / ``mfn_loss_row`` of csrc/inr_device.h, the five entries of csrc/inr_loss.hip) against
the float64 references and derived bounds of tests/loss_cases.py (``-m gpu``): every kind at the partition edges of the
64- and 256-block reductions and on the edge rows, per entry; the rows that are not finite; the same rows through the two
fused fp32 SIREN kernels.  tests/test_gpu_aux_bits.py holds the bytes of these entries, this module says what they have
to be.  Entries are called through ctypes, as tests/aux_bits_cases.py calls them.

Every test prints its largest error / bound and records it through conftest.record_parity under ``loss_family:<key>``
(tools/loss_margins.py merges a run's records into profiles/loss_family_margins.json, the table {key: largest ratio});
a value above 1 fails the test."""
import ctypes as Ct
import os

import numpy as np
import pytest
import torch

import aux_bits_cases as A
import loss_cases as C
import step_tail_cases as S
from aux_bits_cases import dev, rnd

pytestmark = pytest.mark.gpu


def _lib():
    from inr_mi355x import _lib as L
    return L, L.load()


def _record(key, value):
    from conftest import record_parity
    print(f"{key}: worst error / bound = {value:.3f}")
    record_parity("loss_family:" + key, ratio=value)


def _desc(kind, count, hdr_A=C.HDR_A):
    L, _ = _lib()
    return L.LossDesc(kind=C.KINDS[kind], eps=C.EPS, sigma=2.0, factor=C.FACTOR, inv_count=1.0 / count, hdr_A=hdr_A)


def _nan(shape):
    return torch.full(shape, float("nan"), device="cuda")


def _loss_buf(start=0.0):
    L, _ = _lib()
    w = torch.zeros(L.LOSS_WORDS, device="cuda")
    w[0] = start
    return w


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _check(got_loss, got_dout, ref, what):
    """every dout entry written and inside its bound, the loss word inside its bound; returns the worst ratio"""
    assert np.all(np.isfinite(got_dout)), (what, "an entry was not written, or is not finite")
    r = max(C.ratio(got_dout, ref["dout"], ref["dout_bound"]), C.ratio(got_loss, ref["loss"], ref["loss_bound"]))
    assert r <= 1.0, (what, r, C.ratio(got_loss, ref["loss"], ref["loss_bound"]))
    return r


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- inr_loss_grad --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(C.KINDS))
def test_loss_grad(kind):
    """every size of the 64-block partition (empty trailing blocks, per = 257: a lane's second trip), every mask"""
    L, lib = _lib()
    worst = 0.0
    for B in C.SIZES:
        y, t, _ = C.rows(kind, B)
        yd, td = dev(y), dev(t)
        for tag in C.MASKS:
            m, count = C.mask_of(tag, B)
            md = None if m is None else dev(m)
            ref = C.loss_grad_ref(kind, y, t, m, count)
            loss, dout = _loss_buf(), _nan((B, 2))
            ld = _desc(kind, count)
            L.check(lib.inr_loss_grad(Ct.byref(ld), yd.data_ptr(), td.data_ptr(), None, _ptr(md), B, loss.data_ptr(),
                                      dout.data_ptr(), A._stream()))
            got = _np(dout)
            worst = max(worst, _check(_np(loss)[0], got, ref, (kind, B, tag)))
            if m is not None:
                assert not got[m == 0].any(), (kind, B, tag, "an unsampled row is not exactly 0")
    _record(f"loss_grad/{kind}", worst)


@pytest.mark.parametrize("kind", ["hdr", "msle"])
def test_a_row_that_is_not_finite_stays_in_its_row(kind):
    """one row whose float64 loss is +inf (hdr, y == t) or NaN (msle, y < -1): the loss word is not finite, that row's dout
    is NaN, every other row stays inside its bound"""
    L, lib = _lib()
    y, t, bad = C.nonfinite_rows(kind)
    B = len(y)
    ref = C.loss_grad_ref(kind, y, t, None, B, bad=bad)
    loss, dout = _loss_buf(), _nan((B, 2))
    ld = _desc(kind, B)
    yd, td = dev(y), dev(t)
    L.check(lib.inr_loss_grad(Ct.byref(ld), yd.data_ptr(), td.data_ptr(), None, None, B, loss.data_ptr(),
                              dout.data_ptr(), A._stream()))
    got, word = _np(dout), _np(loss)[0]
    assert not np.isfinite(word)
    assert np.isnan(got[bad]).any(axis=1).all()
    r = C.ratio(got[~bad], ref["dout"][~bad], ref["dout_bound"][~bad])
    assert r <= 1.0, r
    _record(f"loss_grad_nonfinite/{kind}", r)


# ---- inr_loss_grad_multi --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NH", C.HEADS)
def test_loss_grad_multi(NH):
    """every kind, size and mask; sampled rows per head, the consistency term on every row with dist exactly on and one fp32 step
    outside a bound, an empty pair, one and two channels"""
    L, lib = _lib()
    worst = {}
    for kind in C.KINDS:
        scale = 0.5 if kind == "logspace" else 1.0
        for B in C.SIZES:
            ys, t, dist = C.multi_rows(kind, NH, B)
            ysd, td, dd = dev(ys), dev(t), dev(dist)
            for tag in C.MASKS:
                m, count = C.mask_of(tag, B)
                md = None if m is None else dev(m)
                for chan in (1, 2):
                    cons = C.Cons(0.1, chan, C.DIST_BOUNDS) if NH > 1 else None
                    ref = C.multi_ref(kind, ys, t, dist, m, count, scale, cons)
                    ld = _desc(kind, count)
                    ld.scale = scale if scale != 1.0 else 0.0  # 0 means 1
                    if cons is not None:
                        ld.cons_w, ld.cons_chan = cons.w, chan
                        for i in range(4):
                            ld.cons_lo[i], ld.cons_hi[i] = float(cons.lo[i]), float(cons.hi[i])
                            ld.cons_inv[i] = cons.inv(i, dist) if i + 1 < NH else 0.0
                    loss, douts = _loss_buf(), _nan((NH, B, 2))
                    L.check(lib.inr_loss_grad_multi(Ct.byref(ld), ysd.data_ptr(), td.data_ptr(), dd.data_ptr(), _ptr(md), NH,
                                                    B, loss.data_ptr(), douts.data_ptr(), A._stream()))
                    r = _check(_np(loss)[0], _np(douts), ref, (kind, NH, B, tag, chan))
                    worst[kind] = max(worst.get(kind, 0.0), r)
                    if cons is None and m is not None:
                        assert not _np(douts)[:, m == 0].any()
                    if cons is None:
                        break  # (one head: no consistency term, the channel count changes nothing)
    for kind, r in worst.items():
        _record(f"loss_grad_multi/heads{NH}/{kind}", r)


# ---- inr_tv_grad, inr_loss_tv_grad ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.TV_SHAPES, ids=lambda s: "_".join(map(str, s)))
def test_tv_and_loss_tv(shape):
    """inr_tv_grad adds into a known vector and a loss word of 0.25; inr_loss_tv_grad writes, for every kind under every
    mask; and the one-pass entry agrees with inr_loss_grad followed by inr_tv_grad inside the sum of their bounds"""
    L, lib = _lib()
    R, R_own, W, H = shape
    n = R * W
    own = np.arange(n) < R_own * W
    worst = {}
    for kind in C.KINDS:
        y, t, _ = C.tv_rows(kind, R, R_own, W)
        yd, td = dev(y), dev(t)
        img = y.reshape(R, W, 2)
        if kind == "l2":
            pre = rnd(n * 2, 16, 0.1).reshape(R, W, 2)
            ref = C.tv_ref(img, R_own, W, H, C.TV_WEIGHT, pre, 0.25)
            loss, dout = _loss_buf(0.25), dev(pre)
            L.check(lib.inr_tv_grad(yd.data_ptr(), R, R_own, W, H, Ct.c_float(float(C.TV_WEIGHT)), loss.data_ptr(),
                                    dout.data_ptr(), A._stream()))
            worst["tv"] = _check(_np(loss)[0], _np(dout), ref, (shape, "tv"))
        for tag in C.MASKS:
            m, _ = C.mask_of(tag, n)
            count = n if m is None else max(int((m != 0)[own].sum()), 1)
            md = None if m is None else dev(m)
            ref = C.loss_tv_ref(kind, y, t, m, count, R, R_own, W, H, C.TV_WEIGHT)
            ld = _desc(kind, count)
            loss, dout = _loss_buf(), _nan((n, 2))
            L.check(lib.inr_loss_tv_grad(Ct.byref(ld), yd.data_ptr(), td.data_ptr(), _ptr(md), R, R_own, W, H,
                                         Ct.c_float(float(C.TV_WEIGHT)), loss.data_ptr(), dout.data_ptr(), A._stream()))
            one_loss, one = _np(loss)[0], _np(dout)
            worst[kind] = max(worst.get(kind, 0.0), _check(one_loss, one, ref, (shape, kind, tag)))
            # dispatch: inr_loss_grad on the owned rows (the caller zeroes the halo row's mask), then inr_tv_grad on top
            m2 = (own if m is None else (m != 0) & own).astype(np.uint8)
            ref1 = C.loss_grad_ref(kind, y, t, m2, count)
            loss2, dout2 = _loss_buf(), _nan((n, 2))
            m2d = dev(m2)
            L.check(lib.inr_loss_grad(Ct.byref(ld), yd.data_ptr(), td.data_ptr(), None, m2d.data_ptr(), n,
                                      loss2.data_ptr(), dout2.data_ptr(), A._stream()))
            step1, word1 = _np(dout2).copy(), float(_np(loss2)[0])
            L.check(lib.inr_tv_grad(yd.data_ptr(), R, R_own, W, H, Ct.c_float(float(C.TV_WEIGHT)), loss2.data_ptr(),
                                    dout2.data_ptr(), A._stream()))
            ref2 = C.tv_ref(img, R_own, W, H, C.TV_WEIGHT, step1.reshape(R, W, 2), word1)
            two, two_loss = _np(dout2), _np(loss2)[0]
            assert np.all(np.abs(one.astype(np.float64) - two) <= ref["dout_bound"] + ref1["dout_bound"]
                          + ref2["dout_bound"].reshape(n, 2)), (shape, kind, tag)
            assert abs(float(one_loss) - float(two_loss)) <= ref["loss_bound"] + ref1["loss_bound"] + ref2["loss_bound"]
    for k, r in worst.items():
        _record(f"tv/{k}" if k == "tv" else f"loss_tv/{k}", r)


# ---- inr_center_pairs_grad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PAIR_N)
def test_center_pairs(n):
    """adds into a known vector and a loss word of 0.25; a pair row at the origin gets gradient 0, pairs with an index of -1,
    B or 10^9 are ignored, rows in no pair keep their bits"""
    L, lib = _lib()
    B = C.PAIR_B
    y, t, ia, ib = C.pair_rows(n)
    pre = rnd(B * 2, 19, 0.1).reshape(B, 2)
    ref = C.pairs_ref(y, t, ia, ib, C.PAIR_WEIGHT, pre, 0.25)
    loss, dout = _loss_buf(0.25), dev(pre)
    yd, td, iad, ibd = dev(y), dev(t), dev(ia), dev(ib)
    L.check(lib.inr_center_pairs_grad(yd.data_ptr(), td.data_ptr(), iad.data_ptr(), ibd.data_ptr(), n, B,
                                      Ct.c_float(float(C.PAIR_WEIGHT)), loss.data_ptr(), dout.data_ptr(), A._stream()))
    got = _np(dout)
    r = _check(_np(loss)[0], got, ref, n)
    untouched = ref["dout_bound"].sum(axis=1) == 0
    assert got[untouched].tobytes() == pre[untouched].tobytes()
    _record(f"center_pairs/n{n}", r)


# ---- the same rows through the fused kernels ------------------------------------------------------------------------
@pytest.mark.parametrize("b", C.FUSED_OUT, ids=["b0", "b1"])
@pytest.mark.parametrize("plan", ["siren32", "siren256"])
def test_fused_rows(plan, b):
    """a SIREN whose last layer has zero weights and bias b outputs y = b on every row, so the targets alone place each
    row on an edge: the logged loss and the last layer's bias gradient (sum over rows of g) of inr_train_step lie inside
    the summed bounds of the float64 reference -- width 32 (inr_mlp_kernel, one block) and width 256 behind the gauss
    encoder (the row-split kernel), B = 129, every kind"""
    from inr_mi355x import _lib as L
    from inr_mi355x.engine import LossSpec
    old = {k: os.environ.pop(k, None) for k in ("INR_PACK_BY_IMAGE", "INR_RS")}
    try:
        eng = A._engine(plan)
        B = C.FUSED_B
        info = L.StepInfo()
        L.check(eng.lib.inr_plan_step_info(eng.plan, B, Ct.byref(info)))
        assert info.row_split == (1 if plan == "siren256" else 0)
        tensors = S.tensors_of(plan)
        (wo, wn), (bo, bn) = tensors[-2], tensors[-1]
        assert bn == 2 and wn == 2 * (256 if plan == "siren256" else 32) and bo + bn == eng.n_params
        p0 = rnd(eng.n_params, 1, 0.1)
        p0[wo:wo + wn] = 0.0
        p0[bo:bo + 2] = np.asarray(b, dtype=np.float32)
        eng.bind(dev(p0).clone())
        x = dev(rnd(B * 3, 2).reshape(B, 3))
        enc_B = dev(rnd(eng.in_features // 2 * 3, 3, 2.0).reshape(-1, 3))
        for kind in C.KINDS:
            t = C.fused_targets(kind, b)
            ref = C.fused_ref(kind, b, t)
            eng.grads.zero_()
            loss = eng.train_step(x, enc_B, dev(t), LossSpec(C.KINDS[kind], C.EPS, 2.0, C.FACTOR, 3000), hdr_A=C.HDR_A)
            torch.cuda.synchronize()
            word, bias = float(loss.item()), eng.grads[bo:bo + 2].cpu().numpy()
            r = max(C.ratio(word, ref["loss"], ref["loss_bound"]), C.ratio(bias, ref["bias"], ref["bias_bound"]))
            print(f"{plan} {kind} b = {b}: loss {word!r} (ref {ref['loss']!r}), bias gradient {bias} (ref {ref['bias']})")
            assert r <= 1.0, (plan, kind, b, r)
            _record(f"fused/{plan}/{kind}", r)
    finally:
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v
