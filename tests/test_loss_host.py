"""The references and bounds of tests/loss_cases.py, checked without a GPU: every float64 reference against
torch.autograd on the oracle's functions in float64; the fp32 restatement of every entry inside its derived bound on
every shipped input, kind and mask; the bounds tight enough to be of use; and twelve deliberately wrong fp32
implementations, each of which leaves the bound at the sizes and shapes where it can.  tests/test_gpu_loss.py holds the kernels to the same references."""
import numpy as np
import pytest
import torch

import loss_cases as C
import oracle as O
from aux_bits_cases import rnd

OPTS = dict(hdr_eps=C.EPS, hdr_ff_sigma=2.0, hdr_ff_factor=C.FACTOR, min_sample=4)
f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def _close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert np.all(err <= rel * np.abs(want)), (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))


def _kcoords(n, far=False):
    k = np.zeros((n, 3))
    k[:, 1], k[:, 2] = (2.0, 0.0) if far else (rnd(n, 40, 1.0), rnd(n, 41, 1.0))
    return f64(k)


def _oracle(kind, y, t, kc):
    if kind == "l2":
        return O.loss_l2_half(y, t)
    if kind == "l1":
        return O.loss_l1_half(y, t)
    if kind == "tanh":
        return O.loss_tanh(y, t)[0]
    if kind == "logspace":
        return O.loss_logspace(y, t, OPTS)
    if kind == "msle":
        return 0.5 * O.loss_msle(y, t)
    if kind == "hdr":
        return O.loss_hdr(y, t, kc, OPTS)[0]
    return O.loss_center(y, t, kc, OPTS)[0]  # kcoords outside both bands: the pointwise part alone


# ---- anchor ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(C.KINDS))
def test_rows_are_the_oracle_in_float64(kind):
    """value and gradient of every kind, on the random rows and on every finite edge row, masked and unmasked.  The
    comparison is per row with the row alone in the batch as well (count = 1), so no edge row hides in a sum."""
    seen = set()
    for B in C.SIZES:
        y, t, names = C.rows(kind, B)
        seen |= set(names.values())
        sub = np.arange(B) if B <= 257 else np.array(sorted(names))
        y, t = y[sub], t[sub]
        n = len(sub)
        for tag in ("none", "half", "single"):
            m, _ = C.mask_of(tag, n)
            keep = np.ones(n, dtype=bool) if m is None else m != 0
            count = int(keep.sum())
            kc = _kcoords(count, far=(kind == "center"))
            A = float(torch.mean((1.0 - torch.exp(-(kc[:, 1] ** 2 + kc[:, 2] ** 2) / (2 * 2.0 ** 2))) ** 2))
            yt = f64(y[keep]).requires_grad_(True)
            loss = _oracle(kind, yt, f64(t[keep]), kc)
            (grad,) = torch.autograd.grad(loss, yt)
            ref = C.loss_grad_ref(kind, y, t, m, count, hdr_A=A)
            _close(ref["loss"], float(loss.detach()), (kind, B, tag, "loss"))
            _close(ref["dout"][keep], grad.numpy(), (kind, B, tag, "dout"), rel=1e-12)
            assert not ref["dout"][~keep].any() and not ref["dout_bound"][~keep].any()
        for r in range(n):
            yt = f64(y[r:r + 1]).requires_grad_(True)
            kc = _kcoords(1, far=True)
            A = float((1.0 - np.exp(-4.0 / 8.0)) ** 2)
            loss = _oracle(kind, yt, f64(t[r:r + 1]), kc)
            (grad,) = torch.autograd.grad(loss, yt)
            ref = C.loss_grad_ref(kind, y[r:r + 1], t[r:r + 1], None, 1, hdr_A=A)
            _close(ref["loss"], float(loss.detach()), (kind, B, r, "row loss"))
            _close(ref["dout"], grad.numpy(), (kind, B, r, "row dout"))
    want = {e[0] for e in C.EDGES if (kind, e[0]) not in C.NOT_FINITE}
    assert seen == want, want - seen


def test_nonfinite_rows_are_not_finite_in_float64():
    for kind in ("hdr", "msle"):
        y, t, bad = C.nonfinite_rows(kind)
        r = int(np.flatnonzero(bad)[0])
        yt = f64(y[r:r + 1]).requires_grad_(True)
        loss = _oracle(kind, yt, f64(t[r:r + 1]), _kcoords(1))
        (grad,) = torch.autograd.grad(loss, yt)
        assert not np.isfinite(float(loss.detach())) and np.isnan(grad.numpy()).any(), kind
        if kind == "hdr":
            assert float(loss.detach()) == np.inf
        ref = C.loss_grad_ref(kind, y, t, None, len(y), bad=bad)
        assert np.isnan(ref["dout"][r]).all() and np.isfinite(ref["dout"][~bad]).all() and np.isfinite(ref["dout_bound"][~bad]).all()
        lw, d = C.loss_grad_f32(kind, y, t, None, len(y))
        assert not np.isfinite(lw) and np.isnan(d[r]).any()
        assert C.ratio(d[~bad], ref["dout"][~bad], ref["dout_bound"][~bad]) <= 1.0


def _cons(chan):
    return C.Cons(0.1, chan, C.DIST_BOUNDS)


@pytest.mark.parametrize("chan", [1, 2])
def test_multi_head_is_the_oracle_in_float64(chan):
    """sum_k scale loss_fn(head k) on the sampled rows + cons_w ConsistencyLoss on every row; dist [B] compares rows,
    dist [B, 1] channel 0 only; pair 1 of DIST_BOUNDS is empty and skipped"""
    B, NH, scale = 257, 4, 0.5
    for kind in ("l2", "logspace"):
        ys, t, dist = C.multi_rows(kind, NH, B)
        cons = _cons(chan)
        assert cons.inv(1, dist) == 0.0 and cons.inv(0, dist) != 0.0 and cons.inv(2, dist) != 0.0
        m, count = C.mask_of("half", B)
        keep = m != 0
        heads = [f64(ys[k]).requires_grad_(True) for k in range(NH)]
        d = torch.from_numpy(dist.copy())  # fp32, compared with fp32 bounds as the kernel compares
        bounds = [(torch.tensor(lo), torch.tensor(hi)) for lo, hi in zip(cons.lo, cons.hi)]
        loss = sum(scale * _oracle(kind, h[keep], f64(t[keep]), None) for h in heads)
        loss = loss + 0.1 * O.loss_consistency(heads, d if chan == 2 else d[:, None], bounds)
        grads = torch.autograd.grad(loss, heads)
        ref = C.multi_ref(kind, ys, t, dist, m, count, scale, cons)
        _close(ref["loss"], float(loss.detach()), (kind, chan, "loss"))
        for k in range(NH):
            _close(ref["dout"][k], grads[k].numpy(), (kind, chan, k))
        # the edge values of dist: exactly lo and exactly hi are NOT compared, one fp32 step outside is
        rows0 = cons.rows(0, dist)
        assert not rows0[dist == cons.lo[0]].any() and not rows0[dist == cons.hi[0]].any()
        assert (dist == cons.lo[0]).any() and (dist == cons.hi[0]).any()
        assert rows0[dist == np.nextafter(cons.lo[0], np.float32(-1))].all() and (dist == np.nextafter(cons.lo[0], np.float32(-1))).any()
        assert rows0[dist == np.nextafter(cons.hi[0], np.float32(2))].all() and (dist == np.nextafter(cons.hi[0], np.float32(2))).any()


def test_tv_is_the_oracle_in_float64():
    """R = R_own = H is tv_loss itself; slabs of R_own rows with a halo row each sum to it, loss and gradient"""
    for (H, W, own) in ((2, 2, 2), (8, 5, 2), (7, 5, 7), (7, 5, 3)):
        y, _, _ = C.tv_rows("l2", H, H, W)
        img = y.reshape(H, W, 2)
        it = f64(img).requires_grad_(True)
        loss = O.loss_tv(it, float(C.TV_WEIGHT))
        (grad,) = torch.autograd.grad(loss, it)
        total, g = 0.0, np.zeros((H, W, 2))
        for y0 in range(0, H, own):
            r_own = min(own, H - y0)
            R = min(r_own + 1, H - y0)
            ref = C.tv_ref(img[y0:y0 + R], r_own, W, H, C.TV_WEIGHT, np.zeros((R, W, 2), dtype=np.float32), 0.0)
            total += ref["loss"]
            g[y0:y0 + R] += ref["dout"]
        _close(total, float(loss.detach()), (H, W, own, "loss"))
        _close(g, grad.numpy(), (H, W, own, "grad"), rel=1e-12)


def test_pairs_are_the_oracle_in_float64(monkeypatch):
    """loss_center with the pairs given: its two torch.randperm draws return the pairs' order, the a rows lie in the inner
    disc of band 1, the b rows in its ring, no row in band 2's ring; hdr_eps = 1e3 makes the pointwise part (subtracted
    through its own anchored reference) a 1e-9 of the pair term"""
    n, B = 65, C.PAIR_B
    y, t, ia, ib = C.pair_rows(n)
    ok = (ia >= 0) & (ia < B) & (ib >= 0) & (ib < B)
    a, b = ia[ok], ib[ok]
    assert len(a) == n - 2
    sub = np.concatenate([a, b])  # the batch the oracle sees: inner rows first
    kc = np.zeros((len(sub), 3))
    kc[:len(a), 1], kc[len(a):, 1] = 0.2, 0.6  # d2 = 0.04 <= 0.1 | 0.1 < 0.36 <= 0.5
    draws = [torch.arange(len(a)), torch.arange(len(b))]
    monkeypatch.setattr(torch, "randperm", lambda k: draws.pop(0)[:k])
    opts = dict(OPTS, hdr_eps=1e3, min_sample=len(a))
    yt = f64(y[sub]).requires_grad_(True)
    loss = O.loss_center(yt, f64(t[sub]), f64(kc), opts)[0]
    (grad,) = torch.autograd.grad(loss, yt)
    assert not draws
    A = float(np.mean((1.0 - np.exp(-kc[:, 1] ** 2 / 8.0)) ** 2))
    point = C.loss_grad_ref("center", y[sub], t[sub], None, len(sub), eps=1e3, hdr_A=A)
    pre = np.zeros((B, 2), dtype=np.float32)
    ref = C.pairs_ref(y, t, a, b, C.PAIR_WEIGHT, pre, 0.0)
    w32 = float(C.PAIR_WEIGHT) / 0.1  # the entry takes the weight as fp32; the oracle's is the double 0.1
    _close(ref["loss"] / w32, float(loss.detach()) - point["loss"], "pair loss", rel=1e-9)
    got = ref["dout"][sub] / w32
    want = grad.numpy() - point["dout"]
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-20)
    origin = ~y[sub].any(axis=1)
    assert origin.sum() == 2 and not got[origin].any()
    # the pairs outside [0, B) change nothing but n: the same sums, divided by n = 65 instead of 63
    full = C.pairs_ref(y, t, ia, ib, C.PAIR_WEIGHT, pre, 0.0)
    _close(full["loss"] * n, ref["loss"] * (n - 2), "n stays n")
    _close(full["dout"] * n, ref["dout"] * (n - 2), "n stays n")


# ---- the fp32 restatement inside the bounds; the bounds of use ---------------------------------------------------------
def _cap(d, b, edge, inv_count, kind, what):
    """the usefulness cap of the bounds on dout [B, 2] (d reference, b bound): of the entries of the random rows 95 % are
    within 1e-4 relative, edge rows ({row: name}) within 1e-2 of max(|reference|, inv_count), but for the rows that
    loss_cases.ILL_CONDITIONED names"""
    B = len(d)
    rows = np.array([r for r in range(B) if r not in edge], dtype=int)
    if len(rows):
        frac = float((b[rows] <= 1e-4 * np.abs(d[rows])).mean())
        assert frac >= 0.95, (what, frac)
    for r, name in edge.items():
        if (kind, name) in C.ILL_CONDITIONED:
            continue
        assert np.all(b[r] <= 1e-2 * np.maximum(np.abs(d[r]), inv_count)), (what, r, name)


def _inside(got, ref):
    return max(C.ratio(got[1], ref["dout"], ref["dout_bound"]), C.ratio(got[0], ref["loss"], ref["loss_bound"]))


@pytest.mark.parametrize("kind", list(C.KINDS))
def test_loss_grad_fp32_within_bound(kind):
    """If this fails the derivation in loss_cases.py's docstring is wrong: correct the analysis."""
    worst = 0.0
    for B in C.SIZES:
        y, t, names = C.rows(kind, B)
        for tag in C.MASKS:
            m, count = C.mask_of(tag, B)
            ref = C.loss_grad_ref(kind, y, t, m, count)
            r = _inside(C.loss_grad_f32(kind, y, t, m, count), ref)
            assert r <= 1.0, (kind, B, tag, r)
            worst = max(worst, r)
            if m is not None:
                assert not ref["dout"][m == 0].any() and not ref["dout_bound"][m == 0].any()
            _cap(ref["dout"], ref["dout_bound"], names, 1.0 / count, kind, (kind, B, tag))
            if tag == "none":
                assert ref["loss_bound"] <= 1e-5 * abs(ref["loss"])
    print(f"{kind}: worst |fp32 - float64| / bound = {worst:.3f}")
    assert worst > 0.01 or kind == "l1"  # not slack by orders of magnitude (l1's gradient is one rounded constant)


@pytest.mark.parametrize("NH", C.HEADS)
def test_multi_fp32_within_bound(NH):
    """every kind, size, mask and channel count; the cap on every head's dout (edge rows: those of ``rows`` and the rows
    whose dist sits on or next to a bound)"""
    for kind in C.KINDS:
        scale = 0.5 if kind == "logspace" else 1.0
        for B in C.SIZES:
            ys, t, dist = C.multi_rows(kind, NH, B)
            names = C.rows(kind, B)[2]
            for tag in C.MASKS:
                m, count = C.mask_of(tag, B)
                for chan in (1, 2):
                    cons = _cons(chan) if NH > 1 else None
                    ref = C.multi_ref(kind, ys, t, dist, m, count, scale, cons)
                    r = _inside(C.multi_f32(kind, ys, t, dist, m, count, scale, cons), ref)
                    assert r <= 1.0, (kind, NH, B, tag, chan, r)
                    for k in range(NH):
                        _cap(ref["dout"][k], ref["dout_bound"][k], names, 1.0 / count, kind, (kind, NH, B, tag, chan, k))


@pytest.mark.parametrize("shape", C.TV_SHAPES, ids=lambda s: "_".join(map(str, s)))
def test_tv_fp32_within_bound(shape):
    R, R_own, W, H = shape
    n = R * W
    for kind in C.KINDS:
        y, t, names = C.tv_rows(kind, R, R_own, W)
        img = y.reshape(R, W, 2)
        if kind == "l2":
            pre = rnd(n * 2, 16, 0.1).reshape(R, W, 2)
            ref = C.tv_ref(img, R_own, W, H, C.TV_WEIGHT, pre, 0.25)
            assert _inside(C.tv_f32(img, R_own, W, H, C.TV_WEIGHT, pre, 0.25), ref) <= 1.0
            # at most four signed coefficients on top of the pre-filled value: a handful of roundings of ITS size
            assert np.all(ref["dout_bound"] <= 8 * C.U * (np.abs(pre) + 4 * max(C.tv_coeffs(C.TV_WEIGHT, W, H))))
            assert ref["loss_bound"] <= 1e-5 * abs(ref["loss"])
        for tag in C.MASKS:
            m, _ = C.mask_of(tag, n)
            count = n if m is None else max(int((m != 0)[:R_own * W].sum()), 1)
            ref = C.loss_tv_ref(kind, y, t, m, count, R, R_own, W, H, C.TV_WEIGHT)
            r = _inside(C.loss_tv_f32(kind, y, t, m, count, R, R_own, W, H, C.TV_WEIGHT), ref)
            assert r <= 1.0, (shape, kind, tag, r)
            if tag in ("none", "half"):
                _cap(ref["dout"], ref["dout_bound"], names, 1.0 / count, kind, (shape, kind, tag))
            # a row without a pointwise gradient holds TV terms alone, and there cw - ch (a 300th of either at W = 259,
            # H = 300) is ill-conditioned in fp32 whatever the inputs: no relative cap, but the absolute one of the
            # analysis -- two stored coefficients, at most three roundings of sums no larger than 2 cw + 2 ch
            keep = np.zeros(n, dtype=bool) if m is None else (m == 0)
            keep[R_own * W:] = True
            cw, ch = C.tv_coeffs(C.TV_WEIGHT, W, H)
            assert np.all(ref["dout_bound"][keep] <= 8 * C.U * (cw + ch)), (shape, kind, tag)


@pytest.mark.parametrize("n", C.PAIR_N)
def test_pairs_fp32_within_bound(n):
    y, t, ia, ib = C.pair_rows(n)
    pre = rnd(C.PAIR_B * 2, 19, 0.1).reshape(-1, 2)
    ref = C.pairs_ref(y, t, ia, ib, C.PAIR_WEIGHT, pre, 0.25)
    assert _inside(C.pairs_f32(y, t, ia, ib, C.PAIR_WEIGHT, pre, 0.25), ref) <= 1.0
    touched = np.zeros(C.PAIR_B, dtype=bool)
    ok = (ia >= 0) & (ia < C.PAIR_B) & (ib >= 0) & (ib < C.PAIR_B)
    touched[ia[ok]] = touched[ib[ok]] = True
    assert not ref["dout_bound"][~touched].any() and np.array_equal(ref["dout"][~touched], pre[~touched].astype(np.float64))
    frac = float((ref["dout_bound"][touched] <= 1e-4 * np.abs(ref["dout"][touched])).mean())
    assert frac >= 0.95, frac
    assert ref["loss_bound"] <= 1e-5 * abs(ref["loss"])


def test_fold32_is_the_naive_partition():
    """fold32 against a per-block, per-lane loop on 300 terms over 64 blocks and on 70000 over 256 (second trips)"""
    for n, nb, tree in ((300, 64, False), (70000, 256, True)):
        x = rnd(n, 50, 1.0)
        per = -(-n // nb)
        parts = []
        for b in range(nb):
            lanes = [np.float32(0)] * 256
            for r in range(b * per, min(b * per + per, n)):
                lanes[(r - b * per) % 256] = np.float32(lanes[(r - b * per) % 256] + x[r])
            s = 128
            while s:
                for k in range(s):
                    lanes[k] = np.float32(lanes[k] + lanes[k + s])
                s //= 2
            parts.append(lanes[0])
        if tree:
            s = nb // 2
            while s:
                for k in range(s):
                    parts[k] = np.float32(parts[k] + parts[k + s])
                s //= 2
            want = parts[0]
        else:
            want = np.float32(0)
            for p in parts:
                want = np.float32(want + p)
        assert C.fold32(x, nb, tree).tobytes() == np.float32(want).tobytes()


# ---- mutations ------------------------------------------------------------------------------------------------------
def _escapes(kind, B, tag="none", post=None, **kw):
    """does a wrong fp32 inr_loss_grad leave the bound on the shipped input of size B?"""
    y, t, _ = C.rows(kind, B)
    m, count = C.mask_of(tag, B)
    ref = C.loss_grad_ref(kind, y, t, m, count)
    if kw.pop("inv_B", False):
        kw["inv"] = 1.0 / B
    if kw.pop("skip_last", False):
        kw["skip_block"] = (B - 1) // (-(-B // C.LOSS_BLOCKS))
    got = C.loss_grad_f32(kind, y, t, m, count, **kw)
    if post is not None:
        got = post(got, y, t, count)
    return _inside(got, ref) > 1.0


def _den_attached(got, y, t, count):
    """logspace with the denominator not detached: dL / d den = -2 L / den flows on through d|y| / dy_o = y_o / |y|"""
    f = np.float32
    e = y - t
    ya = np.sqrt(y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1])
    den = ya + f(C.EPS)
    row = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) * (f(1.0 / count) / (den * den))
    with np.errstate(all="ignore"):
        extra = np.where(ya[:, None] > 0, (f(-2) * row / den)[:, None] * y / ya[:, None], f(0)).astype(f)
    return got[0], got[1] + extra


def test_the_inputs_catch_the_twelve_mutations():
    """each of these slips, restated in fp32, leaves the bound on the shipped inputs -- at the sizes, shapes and kinds named
    here, not merely somewhere; the honest restatement does not (the tests above)"""
    multi = [B for B in C.SIZES if B > 1]
    # 1. eps dropped from the denominator: wherever a row has y = (0, 0), and at the large sizes on the random rows
    for kind in ("logspace", "hdr", "center"):
        hit = [B for B in C.SIZES if _escapes(kind, B, mut="no_eps")]
        assert {257, 16384, 16385} <= set(hit), (kind, hit)
        assert any("y_zero" in C.rows(kind, B)[2].values() for B in hit)
    # 2. denominator not detached
    assert all(_escapes("logspace", B, post=_den_attached) for B in multi)
    # 3. l1: sign(0) = +1 -- at every size that holds a y == t row
    held = [B for B in C.SIZES if {"y_eq_t_one", "y_eq_t_both", "zero_signs_a"} & set(C.rows("l1", B)[2].values())]
    assert len(held) >= 3 and all(_escapes("l1", B, mut="l1_sign0") for B in held)
    # 4. 1 / B in place of 1 / count under a mask: every kind, every size with more than one row, both masks
    for kind in C.KINDS:
        assert all(_escapes(kind, B, "half", inv_B=True) for B in multi), kind
        lone = [B for B in multi if C.rows(kind, B)[2][B - 1] != "y_eq_t_both"]  # (y == t: that row's loss and g are 0)
        assert len(lone) >= len(multi) - 1 and all(_escapes(kind, B, "single", inv_B=True) for B in lone), kind
    # 5. tanh derivative taken at t;  6. msle gradient divided by t + 1
    assert all(_escapes("tanh", B, mut="tanh_at_t") for B in multi)
    assert all(_escapes("msle", B, mut="msle_over_t") for B in multi)
    # 7., 8. consistency compared at dist == lo; its gradient also sent to head i -- at every size that has the dist edges
    for mut in ("cons_le", "cons_both_heads"):
        for NH in (2, 4):
            for B in (63, 65, 257, 16385):
                ys, t, dist = C.multi_rows("l2", NH, B)
                assert (dist == np.float32(C.DIST_BOUNDS[0][0])).any()
                m, count = C.mask_of("half", B)
                ref = C.multi_ref("l2", ys, t, dist, m, count, 1.0, _cons(2))
                _, d = C.multi_f32("l2", ys, t, dist, m, count, 1.0, _cons(2), mut=mut)
                assert C.ratio(d, ref["dout"], ref["dout_bound"]) > 1.0, (mut, NH, B)
    # 9. cw and ch swapped: the gradient of both entries at every shape with cw != ch (the loss words differ by less than
    #    their bounds where W and H are close, and inr_tv_grad's word is 0.25 plus a 1e-5)
    # 10. the halo row adding to the TV loss: the loss word of inr_loss_tv_grad at every shape with a halo row, and
    #    inr_tv_grad's word, which starts at 0.25, where the halo row is a third of the slab
    for mut in ("swap", "halo"):
        shapes = [s for s in C.TV_SHAPES if (s[2] != s[3] if mut == "swap" else s[0] > s[1])]
        assert len(shapes) == (4 if mut == "swap" else 2)
        for R, R_own, W, H in shapes:
            y, t, _ = C.tv_rows("l2", R, R_own, W)
            img, pre = y.reshape(R, W, 2), rnd(R * W * 2, 16, 0.1).reshape(R, W, 2)
            ref = C.tv_ref(img, R_own, W, H, C.TV_WEIGHT, pre, 0.25)
            lw, d = C.tv_f32(img, R_own, W, H, C.TV_WEIGHT, pre, 0.25, mut=mut)
            if mut == "swap":
                assert C.ratio(d, ref["dout"], ref["dout_bound"]) > 1.0, (mut, R, W)
            elif R == 3:
                assert C.ratio(lw, ref["loss"], ref["loss_bound"]) > 1.0, (mut, R, W)
            ref = C.loss_tv_ref("l2", y, t, None, R * W, R, R_own, W, H, C.TV_WEIGHT)
            lw, d = C.loss_tv_f32("l2", y, t, None, R * W, R, R_own, W, H, C.TV_WEIGHT, mut=mut)
            if mut == "swap":
                assert C.ratio(d, ref["dout"], ref["dout_bound"]) > 1.0, (mut, R, W)
            else:
                assert C.ratio(lw, ref["loss"], ref["loss_bound"]) > 1.0, (mut, R, W)
    # 11. the pair gradient's sign on the b row flipped
    for n in C.PAIR_N:
        y, t, ia, ib = C.pair_rows(n)
        pre = rnd(C.PAIR_B * 2, 19, 0.1).reshape(-1, 2)
        ref = C.pairs_ref(y, t, ia, ib, C.PAIR_WEIGHT, pre, 0.25)
        _, d = C.pairs_f32(y, t, ia, ib, C.PAIR_WEIGHT, pre, 0.25, mut="pair_b_sign")
        assert C.ratio(d, ref["dout"], ref["dout_bound"]) > 1.0, n
    # 12. the last non-empty block's rows left out of the loss word: at the sizes with many blocks (65: the last block is
    # row 64 alone; 16385: rows 16191 .. 16384 of block 63), not only where one block is everything
    for kind in C.KINDS:
        for B in (65, 257, 16384, 16385):
            assert _escapes(kind, B, skip_last=True), (kind, B)
