"""inr_focal_loss_grad on the MI355X (``-m gpu``) against the float64 statement of tests/focal_cases.py,
element by element, within bounds DERIVED there from the kernel's operations (nothing fitted to a device); bit equality
where the header promises it: the row that attains n_max (w == 1.0f), aligned against offset pointers, dout = NULL, a
second call."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import focal_cases as FC
from aux_bits_cases import _stream, dev as to_dev
from loss_cases import ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _call(y, t, m, count, alpha=1.0, log_matrix=True, lw=1.0, want_grad=True):
    """(all LOSS_WORDS words, dout) of one call on device tensors"""
    from inr_mi355x import _lib as L
    from inr_mi355x.focal import FocalSpec, focal_loss_grad
    words = torch.full((L.LOSS_WORDS,), -7.0, device=y.device)
    loss, dout = focal_loss_grad(FocalSpec(alpha, log_matrix, lw), y, t, count, mask=m, want_grad=want_grad, loss_out=words)
    torch.cuda.synchronize()
    assert loss.data_ptr() == words.data_ptr()
    return words, dout


def _check(tag, y, t, m, count, alpha, log_matrix, lw, worst, p_max=None):
    """one call against focal_ref; returns (words, dout)"""
    from inr_mi355x import _lib as L
    ref = FC.focal_ref(y, t, m, count, alpha, log_matrix, lw)
    words, dout = _call(to_dev(y), to_dev(t), None if m is None else to_dev(m), count, alpha, log_matrix, lw)
    w, d = words.cpu().numpy(), dout.cpu().numpy()
    r = dict(dout=ratio(d, ref["dout"], ref["dout_bound"]), loss=ratio(w[0], ref["loss"], ref["loss_bound"]),
             n_max=ratio(w[L.FOCAL_NMAX], ref["n_max"], ref["n_max_bound"]))
    print(tag, {k: f"{v:.3f}" for k, v in r.items()}, "loss", w[0], "ref", ref["loss"])
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
        assert v <= 1.0, (tag, k, v)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(d)), tag
    if m is not None:
        assert not d[m == 0].any(), (tag, "an unsampled row is not 0")
    if p_max is not None:  # w == 1.0f exactly: dout = fl(fl(fl(lw 2) e_o) inv), the header's order
        f = np.float32
        e = y[p_max] - t[p_max]
        want = (f(f(lw) * f(2)) * e) * f(1.0 / count)
        assert np.array_equal(d[p_max].view(np.int32), want.astype(f).view(np.int32)), (tag, d[p_max], want)
    return words, dout


@pytest.mark.parametrize("B", FC.SIZES)
def test_kernel_against_float64(dev, B):
    """the largest |e| at row 0, row B - 1 and the first / last row of the first / last non-empty block, the six
    (alpha, log_matrix) combinations taken in turn over the positions; a random mask with the maximum sampled"""
    worst, k = {}, FC.SIZES.index(B)
    y0, t = FC.rows(B)
    for p in FC.max_positions(B):
        y = FC.with_max_at(y0, t, p)
        alpha, lg = FC.COMBOS[k % len(FC.COMBOS)]
        k += 1
        _check(f"B={B} max@{p} a={alpha} log={lg}", y, t, None, B, alpha, lg, 1.0, worst, p_max=p)
        m = FC.random_mask(B)
        m[p] = 1
        _check(f"B={B} max@{p} masked", y, t, m, int(m.sum()), alpha, lg, 0.3, worst, p_max=p)
    from conftest import record_parity
    record_parity(f"focal:kernel/B={B}", **worst)


@pytest.mark.parametrize("alpha, lg", FC.COMBOS)
def test_every_combination(dev, alpha, lg):
    """alpha x log_matrix at B = 1000 (more than one trip of no lane, several blocks), plain and masked"""
    worst = {}
    B = 1000
    y, t = FC.rows(B, seed=3)
    _check(f"a={alpha} log={lg}", y, t, None, B, alpha, lg, 1.0, worst)
    m = FC.random_mask(B)
    _check(f"a={alpha} log={lg} masked", y, t, m, int(m.sum()), alpha, lg, 0.3, worst)
    from conftest import record_parity
    record_parity(f"focal:combo/alpha={alpha},log={int(lg)}", **worst)


def test_tie_masked_maximum_all_masked_and_equal(dev):
    from inr_mi355x import _lib as L
    B, worst = 513, {}
    y0, t = FC.rows(B, seed=5)
    # two rows tie for the maximum (the same e, so the same n to the bit): both get w == 1
    y, t = FC.with_max_at(y0, t, 7), t.copy()
    y[400], t[400] = y[7], t[7]
    words, dout = _check("tie", y, t, None, B, 1.0, True, 1.0, worst, p_max=7)
    assert _bits(dout[400], dout[7]) and bool(dout[7].any())
    # the largest |e| of all in a masked-out row: it does not enter n_max
    y = FC.with_max_at(y0, t, 300)
    m = FC.random_mask(B)
    m[300] = 0
    words, dout = _check("max masked out", y, t, m, int(m.sum()), 1.0, True, 1.0, worst)
    e = (y - t).astype(np.float64)
    n = np.log(np.sqrt((e * e).sum(1)) + 1.0)
    assert n[300] > 1.2 * n[m != 0].max() and float(words[L.FOCAL_NMAX]) < 0.5 * (n[300] + n[m != 0].max())
    # all rows masked: loss 0, every gradient 0, no NaN
    zero = np.zeros(B, dtype=np.uint8)
    words, dout = _call(to_dev(y), to_dev(t), to_dev(zero), 1)
    assert float(words[0]) == 0.0 and float(words[L.FOCAL_NMAX]) == 0.0 and not bool(dout.any())
    assert bool(torch.isfinite(words).all())
    # prediction == target: 0 / 0 -> 0
    for lg in (True, False):
        words, dout = _call(to_dev(t), to_dev(t), None, B, 0.5, lg)
        assert float(words[0]) == 0.0 and float(words[L.FOCAL_NMAX]) == 0.0 and not bool(dout.any())
        assert bool(torch.isfinite(words).all()) and bool(torch.isfinite(dout).all())
    # ... on the sampled rows only: one unsampled row differs
    y = t.copy()
    y[5] += np.float32(0.5)
    m = np.ones(B, dtype=np.uint8)
    m[5] = 0
    words, dout = _call(to_dev(y), to_dev(t), to_dev(m), B - 1)
    assert float(words[0]) == 0.0 and not bool(dout.any())


def test_alignment_null_gradient_and_repeat_change_no_bit(dev):
    """views that start one row into a buffer (8-byte aligned only) give the bits of 16-byte aligned copies; dout = NULL
    gives the same loss_out, every word; so does a second call"""
    for B in (1, 2, 777, 65537):
        y, t = FC.rows(B + 1, seed=7)
        m = FC.random_mask(B + 1)
        m[1] = 1
        yd, td, md = to_dev(y), to_dev(t), to_dev(m)
        count = int(m[1:].sum())
        for mask in (None, md):
            cnt = B if mask is None else count
            mk = lambda v: None if mask is None else v
            a_words, a_dout = _call(yd[1:].clone(), td[1:].clone(), mk(md[1:].clone()), cnt, 0.5, True, 0.3)
            assert yd[1:].data_ptr() % 16 == 8 and yd[1:].clone().data_ptr() % 16 == 0
            b_words, b_dout = _call(yd[1:], td[1:], mk(md[1:]), cnt, 0.5, True, 0.3)
            assert _bits(a_words, b_words) and _bits(a_dout, b_dout), (B, "alignment")
            c_words, none = _call(yd[1:], td[1:], mk(md[1:]), cnt, 0.5, True, 0.3, want_grad=False)
            assert none is None and _bits(c_words, b_words), (B, "dout = NULL")
            d_words, none = _call(yd[1:].clone(), td[1:].clone(), mk(md[1:].clone()), cnt, 0.5, True, 0.3, want_grad=False)
            assert _bits(d_words, a_words), (B, "dout = NULL, aligned")
            e_words, e_dout = _call(yd[1:], td[1:], mk(md[1:]), cnt, 0.5, True, 0.3)
            assert _bits(e_words, b_words) and _bits(e_dout, b_dout), (B, "twice")


def test_loss_out_words_are_laid_out_as_documented(dev):
    """loss_out[0] == ((the partials added in block order) inv) lw to the bit; n_max is the largest of the per-block
    maxima; the words of empty blocks are 0"""
    from inr_mi355x import _lib as L
    B = 65537
    y, t = FC.rows(B, seed=9)
    words, _ = _call(to_dev(y), to_dev(t), None, B, 1.0, True, 0.3)
    w = words.cpu().numpy()
    s = np.float32(0)
    for b in range(L.FOCAL_BLOCKS):
        s = np.float32(s + w[L.FOCAL_PARTIALS + b])
    assert np.float32(np.float32(s * np.float32(1.0 / B)) * np.float32(0.3)) == w[0]
    assert w[L.FOCAL_NMAX] == w[L.FOCAL_MAXIMA:L.FOCAL_MAXIMA + L.FOCAL_BLOCKS].max()
    blocks = FC.block_rows(B)
    assert not w[L.FOCAL_MAXIMA + len(blocks):L.FOCAL_MAXIMA + L.FOCAL_BLOCKS].any()  # empty blocks leave 0, not garbage
    assert not w[L.FOCAL_PARTIALS + len(blocks):L.FOCAL_PARTIALS + L.FOCAL_BLOCKS].any()


def test_bad_arguments_leave_the_outputs_alone(dev):
    from inr_mi355x import _lib as L
    lib = L.load()
    B = 64
    y, t = (to_dev(a) for a in FC.rows(B))
    sent = 123.25
    dout, loss = torch.full((B, 2), sent, device=dev), torch.full((L.LOSS_WORDS,), sent, device=dev)
    good = L.FocalDesc(alpha=1.0, log_matrix=1, loss_weight=1.0, inv_count=1.0 / B)
    desc = lambda **kw: Ct.byref(L.FocalDesc(**dict(dict(alpha=1.0, log_matrix=1, loss_weight=1.0, inv_count=1.0 / B), **kw)))
    p = lambda x: x.data_ptr()
    nan, inf = float("nan"), float("inf")
    calls = [
        (None, p(y), p(t), None, B, p(loss), p(dout)),
        (Ct.byref(good), None, p(t), None, B, p(loss), p(dout)),
        (Ct.byref(good), p(y), None, None, B, p(loss), p(dout)),
        (Ct.byref(good), p(y), p(t), None, B, None, p(dout)),
        (Ct.byref(good), p(y), p(t), None, 0, p(loss), p(dout)),
        (Ct.byref(good), p(y), p(t), None, -5, p(loss), p(dout)),
        (desc(alpha=0.0), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(alpha=-1.0), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(alpha=nan), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(alpha=inf), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(loss_weight=nan), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(loss_weight=inf), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(inv_count=nan), p(y), p(t), None, B, p(loss), p(dout)),
        (desc(inv_count=-inf), p(y), p(t), None, B, p(loss), p(dout)),
        (Ct.byref(good), p(y) + 4, p(t), None, B - 1, p(loss), p(dout)),
        (Ct.byref(good), p(y), p(t) + 4, None, B - 1, p(loss), p(dout)),
        (Ct.byref(good), p(y), p(t), None, B - 1, p(loss), p(dout) + 4),
    ]
    for args in calls:
        assert lib.inr_focal_loss_grad(*args, _stream()) == -1, args
        assert "inr_focal_loss_grad" in L.last_error()
    torch.cuda.synchronize()
    assert bool((dout == sent).all()) and bool((loss == sent).all())
