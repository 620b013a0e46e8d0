"""Cases and references of tests/test_loss_host.py (CPU) and tests/test_gpu_loss.py: the arithmetic of ``loss_row`` and
``mfn_loss_row`` (csrc/inr_device.h) and of the streaming family of csrc/inr_loss.hip (inr_loss_grad, inr_loss_grad_multi,
inr_tv_grad, inr_loss_tv_grad, inr_center_pairs_grad) against float64 statements of what they compute.  A plain module
like step_tail_cases.py, not a conftest.

The references
--------------
Every formula is written ONCE, over a number class: run on ``V`` it gives the float64 reference together with a bound on
|fp32 result - reference|; run on ``F`` it gives the fp32 restatement (every operation rounded to fp32, ``log`` and
``tanh`` taken in float64 and rounded).  tests/test_loss_host.py anchors the float64 values to torch.autograd on the
functions of oracle/inr_oracle.py evaluated in float64, so a slip in a formula here cannot hide in both.

Per sampled row, y = (y0, y1) the output, t the target, inv = 1 / count (count = rows entering the mean), e = y - t,
den = |y| + eps DETACHED (no gradient flows through it), A = hdr_A (passed in):
    l2       loss_l2_half     L = sum_o e_o^2 inv / 4                     g_o = e_o inv / 2
    l1       loss_l1_half     L = sum_o |e_o| inv / 4                     g_o = sign(e_o) inv / 4,  sign(0) = 0
    tanh     loss_tanh        L = sum_o (tanh y_o - tanh t_o)^2 inv / 2   g_o = (tanh y_o - tanh t_o)(1 - tanh^2 y_o) inv
    logspace loss_logspace    L = |e|^2 inv / den^2                       g_o = 2 e_o inv / den^2
    msle     0.5 loss_msle    d_o = log(y_o + 1 + 1e-9) - log(t_o + 1 + 1e-9),   L = sum_o d_o^2 inv / 4
                                                                          g_o = d_o / (y_o + 1 + 1e-9) inv / 2
    hdr      loss_hdr         lg = log(|e| / den),  rq = factor A / den^2,  L = (lg^2 + rq |y|^2) inv
                                                                          g_o = (2 lg e_o / |e|^2 + 2 rq y_o) inv
    center   loss_center's pointwise part (0.1 rel + 0.9 (rel + reg)):  rq = 0.9 factor A inv / den^2
                              L = |e|^2 inv / den^2 + rq |y|^2            g_o = 2 e_o inv / den^2 + 2 rq y_o
Unsampled rows (mask == 0) add nothing and get g = 0.
``multi_ref``    heads k < NH: scale * L on sampled rows, gradient scale * g to head k.  Consistency pair i (heads i,
    i + 1 < NH, skipped when cons_inv[i] == 0) on EVERY row with dist < lo_i or dist > hi_i (strict, fp32 comparison of
    fp32 values): cons_w (y_{i+1,o} - y_{i,o})^2 cons_inv_i over o < cons_chan, gradient 2 cons_w (..) cons_inv_i to
    head i + 1 ONLY (head i is detached).
``tv_ref``       rows [0, R) of a W x H image of which the first R_own are the caller's: cw = weight / (2 H (W - 1)),
    ch = weight / (2 (H - 1) W), computed here from weight, W and H.  Horizontal pairs of the rows r < R_own and the
    vertical pairs (r, r + 1) with r < R_own, r + 1 < R add cw |d| / ch |d| per channel; the gradient of those pairs goes
    to both ends, the halo row (r = R_own < R) included, which adds no loss of its own.
``pairs_ref``    r_p = (|t_a| - |t_b|) - (|y_a| - |y_b|), w = weight / n:  w sum_p r_p^2,  -2 w r_p y_a / |y_a| to row a,
    +2 w r_p y_b / |y_b| to row b, 0 where |y| = 0; a pair with an index outside [0, B) is ignored (n stays n).

The bounds
----------
u = 2^-24.  An exact quantity X is carried with a bound e on |computed - X| (class ``V``); the rules are those of
step_tail_cases.py:
    fp32 input: e = 0        constant c stored as fp32 (eps, inv_count, hdr_A, 0.9, 1e-9, cons_w, cons_inv, cw, ch, w):  e = u |c|
    rounding of a result X:  e' = e + k u (|X| + e)     k = 1 for + - * and fma, k = 2 for sqrt and /
    a + b: e = ea + eb       a * b: e = |a| eb + |b| ea + ea eb       a / b: e = (ea + |a / b| eb) / (|b| - eb)
    sqrt a: e = min(ea / sqrt a, sqrt ea)
    x + 0 with an exact 0, a product with an exact factor +-1, 0, 2, 1/2, 1/4: no rounding
and one more for the two library functions:
    f in {log, tanh}:        e' = sup|f'| e_x + k_f u (|f(x)| + sup|f'| e_x)    sup over [x - e_x, x + e_x]:
                             1 / (x - e_x) for log,  1 - tanh^2(max(|x| - e_x, 0)) for tanh
    K_LOG = K_TANH = 4.  k_f is meant to be twice the max-ulp figure of HIP's math documentation for logf / tanhf; a
    ROCm installation ships no such table (nothing under its share/ or include/ directories states an ulp figure for
    either), so the fallback value 4 is used for both.
Where the compiler contracts a product and a sum into an fma the error only shrinks.  The sign of an fp32 difference of two
fp32 numbers is the sign of the exact difference, so sign(e) and the TV signs are exact.  Every rule is an inequality;
nothing is neglected to first order or fitted to what a device returns.

The loss word: sum over the terms of their bounds, plus gamma(n) sum(|term| + bound) with gamma(n) = n u / (1 - n u) and n
the number of additions on the longest chain: the terms one lane adds (ceil(per / 256) rows, three terms per coordinate
in the loss + TV kernel), 8 levels of the 256-lane tree, then the 64 partials in order (or the 8 levels of
loss_tv_fold_kernel), one more for the entries that add into loss_out[0].  TV gradients are sums of at most four terms
+-cw, +-ch with exact signs: the rounding of the two coefficients (once each, times the net count of its terms: the
terms are multiples of one stored number) and of the additions that can round (``_tv_accumulate``).

The rounding rule holds in the fp32 NORMAL range only: ``V`` asserts that every product, quotient and function value is
exactly 0 or between 2^-120 and 2^100 in magnitude (sums and differences are exact below the normal range).

Inputs
------
``rows(kind, B)``: y and t from aux_bits_cases.rnd at amplitude 0.3 (msle: |.| + 0.05, as the aux-bits case), then the
rows of ``EDGES`` in turn at ``edge_positions``: row 0, row B - 1, first and last row of block 0 and of the last
non-empty block (blocks of per = ceil(B / nblocks) rows), rows 255 / 256 / 257.  The turn continues from one size of
``SIZES`` to the next, so every edge row occurs for every kind.  Rows that are not finite in float64 (hdr with y == t,
msle with y < -1) are kept out of these sets: ``nonfinite_rows``.
"""
import numpy as np

from aux_bits_cases import rnd

U = 2.0 ** -24
TINY = 2.0 ** -120
K_LOG = 4    # no ulp table installed: the fallback value (module docstring)
K_TANH = 4

KINDS = {"l2": 0, "l1": 1, "tanh": 2, "logspace": 3, "hdr": 4, "msle": 5, "center": 6}  # enum inr_loss
EPS, FACTOR, HDR_A = 1e-3, 0.5, 0.37
SIZES = (1, 63, 64, 65, 257, 16384, 16385)
HEADS = (1, 2, 4)
TV_SHAPES = ((2, 2, 2, 2), (3, 2, 5, 8), (7, 7, 5, 7), (129, 128, 3, 200), (254, 254, 259, 300))  # (R, R_own, W, H)
TV_WEIGHT = np.float32(1e-4)
PAIR_N = (1, 64, 65, 16385)
PAIR_B = 20000
PAIR_WEIGHT = np.float32(0.1)
MASKS = ("none", "half", "single", "zero")
LOSS_BLOCKS, LOSS_TV_BLOCKS = 64, 256


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the two number classes -----------------------------------------------------------------------------------------
def _normal(x):
    a = np.abs(x)
    assert np.all((a == 0.0) | ((a > TINY) & (a < 2.0 ** 100))), "an intermediate leaves the fp32 normal range"


class V:
    """exact value x (float64) with a bound e on |fp32 computed value - x|"""
    __slots__ = ("x", "e")

    def __init__(self, x, e=None):
        self.x = np.asarray(x, dtype=np.float64)
        self.e = np.zeros_like(self.x) if e is None else np.asarray(e, dtype=np.float64) + 0.0 * self.x

    inp = classmethod(lambda cls, a: cls(a))
    exact = classmethod(lambda cls, c: cls(c))
    const = classmethod(lambda cls, c: cls(c, U * abs(float(c))))

    @staticmethod
    def _rd(x, e, k=1):
        return e + k * U * (np.abs(x) + e)

    def _is0(self):
        return (self.x == 0.0) & (self.e == 0.0)

    def __add__(self, o):
        x, e = self.x + o.x, self.e + o.e
        return V(x, np.where(self._is0() | o._is0(), e, self._rd(x, e)))

    def __neg__(self):
        return V(-self.x, self.e)

    def __sub__(self, o):
        return self + (-o)

    def __mul__(self, o):
        x = self.x * o.x
        _normal(x)
        return V(x, self._rd(x, np.abs(self.x) * o.e + np.abs(o.x) * self.e + self.e * o.e))

    def __truediv__(self, o):
        assert np.all(np.abs(o.x) > 2.0 * o.e)
        x = self.x / o.x
        _normal(x)
        return V(x, self._rd(x, (self.e + np.abs(x) * o.e) / (np.abs(o.x) - o.e), 2))

    def sqrt(self):
        assert np.all(self.x >= 0.0)
        x = np.sqrt(self.x)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(self.x > 0.0, np.minimum(self.e / x, np.sqrt(self.e)), np.sqrt(self.e))
        return V(x, self._rd(x, e, 2))

    def log(self):
        assert np.all(self.x - self.e > 0.0)
        x = np.log(self.x)
        _normal(x)
        return V(x, self._rd(x, self.e / (self.x - self.e), K_LOG))

    def tanh(self):
        x = np.tanh(self.x)
        _normal(x)
        return V(x, self._rd(x, self.e * (1.0 - np.tanh(np.maximum(np.abs(self.x) - self.e, 0.0)) ** 2), K_TANH))

    def abs(self):
        return V(np.abs(self.x), self.e)

    def sign(self):
        """exact: only ever taken of an fp32 difference of fp32 inputs"""
        assert np.all(self.e <= U * np.abs(self.x))
        return np.sign(self.x)

    def times(self, a):
        """product with an exact factor that needs no rounding (+-1, 0, powers of two; a numpy array or a float)"""
        a = np.asarray(a, dtype=np.float64)
        return V(self.x * a, self.e * np.abs(a))

    def val(self):
        return self.x


class F:
    """an fp32 value; every operation rounds to fp32 (numpy), log and tanh through float64"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = np.asarray(v, dtype=np.float32)

    inp = classmethod(lambda cls, a: cls(a))
    exact = classmethod(lambda cls, c: cls(np.float32(c)))
    const = classmethod(lambda cls, c: cls(np.float32(c)))

    def __add__(self, o):
        with np.errstate(all="ignore"):
            return F(self.v + o.v)

    def __neg__(self):
        return F(-self.v)

    def __sub__(self, o):
        with np.errstate(all="ignore"):
            return F(self.v - o.v)

    def __mul__(self, o):
        with np.errstate(all="ignore"):
            return F(self.v * o.v)

    def __truediv__(self, o):
        with np.errstate(all="ignore"):
            return F(self.v / o.v)

    def sqrt(self):
        with np.errstate(all="ignore"):
            return F(np.sqrt(self.v))

    def log(self):
        with np.errstate(all="ignore"):
            return F(np.log(self.v.astype(np.float64)).astype(np.float32))

    def tanh(self):
        return F(np.tanh(self.v.astype(np.float64)).astype(np.float32))

    def abs(self):
        return F(np.abs(self.v))

    def sign(self):
        return np.sign(self.v).astype(np.float64)

    def times(self, a):
        with np.errstate(all="ignore"):
            return F(self.v * np.asarray(a, dtype=np.float32))

    def val(self):
        return self.v


# ---- one row of loss_row, over either class -------------------------------------------------------------------------
def row_terms(N, kind, y, t, inv, eps=EPS, factor=FACTOR, hdr_A=HDR_A, mut=None):
    """(L, g0, g1) of class N for rows y, t [B, 2] (fp32): the operations of loss_row in its order.  ``inv``: an N
    (1 / count).  ``mut`` names one of the deliberate mistakes of tests/test_loss_host.py (F only)."""
    y = np.asarray(y, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    Y, T = [N.inp(y[:, 0]), N.inp(y[:, 1])], [N.inp(t[:, 0]), N.inp(t[:, 1])]
    one = N.exact(1.0)
    E = [Y[0] - T[0], Y[1] - T[1]]
    L, g = None, []
    add = lambda a, b: b if a is None else a + b
    if kind == "l2":
        s = inv.times(0.5)
        for o in (0, 1):
            L = add(L, (E[o].times(0.5) * E[o]) * s)
            g.append(E[o] * s)
    elif kind == "l1":
        s = inv.times(0.25)
        for o in (0, 1):
            L = add(L, E[o].abs() * s)
            sg = E[o].sign()
            if mut == "l1_sign0":
                sg = np.where(sg == 0.0, 1.0, sg)
            g.append(s.times(sg))
    elif kind == "tanh":
        s = inv.times(0.5)
        for o in (0, 1):
            ty, tt = Y[o].tanh(), T[o].tanh()
            d = ty - tt
            L = add(L, (d * d) * s)
            at = tt if mut == "tanh_at_t" else ty
            g.append((d.times(2.0) * (one - at * at)) * s)
    elif kind == "msle":
        s = inv.times(0.5)
        c9 = N.const(1e-9)
        for o in (0, 1):
            ay, at = (Y[o] + one) + c9, (T[o] + one) + c9
            d = ay.log() - at.log()
            L = add(L, (d.times(0.5) * d) * s)
            g.append((d / (at if mut == "msle_over_t" else ay)) * s)
    else:
        ya2 = Y[0] * Y[0] + Y[1] * Y[1]
        ya = ya2.sqrt()
        den = ya if mut == "no_eps" else ya + N.const(eps)
        ea2 = E[0] * E[0] + E[1] * E[1]
        if kind == "logspace":
            q = inv / (den * den)
            L = ea2 * q
            g = [E[o].times(2.0) * q for o in (0, 1)]
        elif kind == "center":
            q = inv / (den * den)
            rq = ((N.const(0.9) * N.const(factor)) * N.const(hdr_A)) * q
            L = ea2 * q + rq * ya2
            g = [E[o].times(2.0) * q + rq.times(2.0) * Y[o] for o in (0, 1)]
        elif kind == "hdr":
            lg = (ea2.sqrt() / den).log()
            rq = (N.const(factor) * N.const(hdr_A)) / (den * den)
            L = (lg * lg + rq * ya2) * inv
            c1, c2 = (lg.times(2.0) / ea2) * inv, rq.times(2.0) * inv
            g = [c1 * E[o] + c2 * Y[o] for o in (0, 1)]
        else:
            raise KeyError(kind)
    return L, g[0], g[1]


def _sel(n, keep):
    """rows with keep == False become an exact 0"""
    return n.times(np.asarray(keep, dtype=np.float64)) if isinstance(n, V) else F(np.where(keep, n.v, np.float32(0)))


def _safe(y, t, keep):
    """rows that are not kept never reach the formulas in the kernel: give them harmless values"""
    y, t = np.array(y, dtype=np.float32), np.array(t, dtype=np.float32)
    y[~keep], t[~keep] = np.float32(0.25), np.float32(0.5)
    return y, t


def _chain(per, terms_per_row, tree_fold, adds):
    trips = -(-per // 256)
    return trips * terms_per_row + 8 + (8 if tree_fold else LOSS_BLOCKS) + (1 if adds else 0)


def _word(terms, chain, start=0.0):
    """(float64 sum, bound) of a loss word from its V terms (any shapes) and the addition chain's length"""
    s = float(start) + sum(float(t.x.sum()) for t in terms)
    eb = sum(float(t.e.sum()) for t in terms)
    mag = abs(float(start)) + sum(float((np.abs(t.x) + t.e).sum()) for t in terms)
    return s, eb + gamma(chain) * mag


def fold32(terms, nblocks, tree_fold, start=None, skip_block=None):
    """the kernels' summation in fp32: terms [n, m] (row r's m terms in order, 0 where the kernel adds nothing); blocks of
    per = ceil(n / nblocks) rows, lane j adds rows lo + j, lo + j + 256, ... from 0, the 256-lane tree, then the
    partials in order from 0 (``tree_fold``: by the same tree, loss_tv_fold_kernel); ``start``: loss_out[0] is added to"""
    terms = np.asarray(terms, dtype=np.float32)
    terms = terms.reshape(len(terms), -1)
    n, per = len(terms), -(-len(terms) // nblocks)
    part = np.zeros(nblocks, dtype=np.float32)

    def tree(a):
        a = a.copy()
        s = len(a) // 2
        while s > 0:
            a[:s] = a[:s] + a[s:2 * s]
            s //= 2
        return a[0]

    with np.errstate(all="ignore"):
        for b in range(nblocks):
            lo, hi = b * per, min(b * per + per, n)
            if lo >= hi or b == skip_block:
                continue
            lanes = np.zeros(256, dtype=np.float32)
            for r0 in range(lo, hi, 256):
                k = min(256, hi - r0)
                for m in range(terms.shape[1]):
                    lanes[:k] = lanes[:k] + terms[r0:r0 + k, m]
            part[b] = tree(lanes)
        if tree_fold:
            s = tree(part)
        else:
            s = np.float32(0)
            for b in range(nblocks):
                s = np.float32(s + part[b])
        return np.float32(s) if start is None else np.float32(np.float32(start) + s)


# ---- inr_loss_grad --------------------------------------------------------------------------------------------------
def _keep(mask, B):
    return np.ones(B, dtype=bool) if mask is None else np.asarray(mask) != 0


def loss_grad_ref(kind, y, t, mask, count, bad=None, **opts):
    """inr_loss_grad: dict(loss, loss_bound, dout [B, 2], dout_bound).  ``bad``: bool [B], rows whose values are not
    finite: their dout / bound entries are NaN / inf and the loss word has no bound"""
    B = len(y)
    keep = _keep(mask, B)
    fine = keep if bad is None else keep & ~bad
    ys, ts = _safe(y, t, fine)
    L, g0, g1 = (_sel(n, fine) for n in row_terms(V, kind, ys, ts, V.const(1.0 / count), **opts))
    loss, lb = _word([L], _chain(-(-B // LOSS_BLOCKS), 1, False, False))
    dout, db = np.stack([g0.x, g1.x], axis=1), np.stack([g0.e, g1.e], axis=1)
    if bad is not None and np.any(keep & bad):
        dout[keep & bad], db[keep & bad], loss, lb = np.nan, np.inf, np.nan, np.inf
    return dict(loss=loss, loss_bound=lb, dout=dout, dout_bound=db)


def loss_grad_f32(kind, y, t, mask, count, mut=None, inv=None, skip_block=None, **opts):
    """the fp32 restatement: (loss word, dout [B, 2]) as fp32"""
    B = len(y)
    keep = _keep(mask, B)
    ys, ts = _safe(y, t, keep)
    L, g0, g1 = (_sel(n, keep) for n in row_terms(F, kind, ys, ts, F.const(1.0 / count if inv is None else inv), mut=mut, **opts))
    return fold32(L.v, LOSS_BLOCKS, False, skip_block=skip_block), np.stack([g0.v, g1.v], axis=1)


# ---- inr_loss_grad_multi --------------------------------------------------------------------------------------------
class Cons:
    """the consistency fields of a loss descriptor: cons_w, cons_chan, fp32 lo / hi per pair; cons_inv is counted here"""

    def __init__(self, w, chan, bounds):
        self.w, self.chan = w, chan
        self.lo = [np.float32(b[0]) for b in bounds]
        self.hi = [np.float32(b[1]) for b in bounds]

    def rows(self, i, dist, le=False):
        d = np.asarray(dist, dtype=np.float32)
        return ((d <= self.lo[i]) if le else (d < self.lo[i])) | (d > self.hi[i])

    def inv(self, i, dist):
        n = int(self.rows(i, dist).sum()) * self.chan
        return 1.0 / n if n else 0.0


def multi_terms(N, kind, ys, t, dist, keep, count, scale, cons, mut=None):
    """(L, g[k][o]) of class N: mfn_loss_row in its order; ys [NH, B, 2]"""
    NH, B = len(ys), len(t)
    sc = N.exact(scale)  # 0.5 or 1: exact
    L, g = None, []
    for k in range(NH):
        yk, tk = _safe(ys[k], t, keep)
        Lk, g0, g1 = (_sel(n, keep) for n in row_terms(N, kind, yk, tk, N.const(1.0 / count)))
        L = sc * Lk if L is None else L + sc * Lk
        g.append([sc * g0, sc * g1])
    if cons is not None and cons.w != 0.0:
        w = N.const(cons.w)
        for i in range(NH - 1):
            ci = cons.inv(i, dist)
            if ci == 0.0:
                continue
            rows = cons.rows(i, dist, le=(mut == "cons_le"))
            inv = N.const(ci)
            for o in range(cons.chan):
                e = N.inp(ys[i + 1][:, o]) - N.inp(ys[i][:, o])
                L = L + _sel(((w * e) * e) * inv, rows)
                ge = _sel((w.times(2.0) * e) * inv, rows)
                g[i + 1][o] = g[i + 1][o] + ge
                if mut == "cons_both_heads":
                    g[i][o] = g[i][o] - ge
    return L, g


def multi_ref(kind, ys, t, dist, mask, count, scale, cons):
    """inr_loss_grad_multi: dict(loss, loss_bound, dout [NH, B, 2], dout_bound)"""
    B = len(t)
    L, g = multi_terms(V, kind, ys, t, dist, _keep(mask, B), count, scale, cons)
    terms_per_row = len(ys) + (0 if cons is None else (len(ys) - 1) * cons.chan)  # the row's own additions come first
    loss, lb = _word([L], _chain(-(-B // LOSS_BLOCKS), 1, False, False) + terms_per_row)
    return dict(loss=loss, loss_bound=lb, dout=np.stack([np.stack([a.x, b.x], axis=1) for a, b in g]),
                dout_bound=np.stack([np.stack([a.e, b.e], axis=1) for a, b in g]))


def multi_f32(kind, ys, t, dist, mask, count, scale, cons, mut=None):
    L, g = multi_terms(F, kind, ys, t, dist, _keep(mask, len(t)), count, scale, cons, mut=mut)
    return fold32(L.v, LOSS_BLOCKS, False), np.stack([np.stack([a.v, b.v], axis=1) for a, b in g])


# ---- total variation ------------------------------------------------------------------------------------------------
def tv_coeffs(weight, W, H):
    w = float(np.float32(weight))
    return w / (H * (W - 1) * 2.0), w / ((H - 1) * W * 2.0)


def _tv_diffs(img, R_own):
    """TV of rows [0, R) (img [R, W, 2] fp32) as V: (dh, dv, nv): the differences of the horizontal pairs of the rows
    r < R_own [R_own, W - 1, 2] and of the nv = min(R_own, R - 1) vertical pairs (r, r + 1) [nv, W, 2]"""
    nv = min(R_own, img.shape[0] - 1)
    return V.inp(img[:R_own, :-1]) - V.inp(img[:R_own, 1:]), V.inp(img[:nv]) - V.inp(img[1:nv + 1]), nv


def _tv_accumulate(g0, img, cw, ch, nv, sh, sv):
    """g0 [R, W, 2] (V) plus the four sign terms of every element in the kernels' order: + cw sgn(v - right),
    - cw sgn(left - v), + ch sgn(v - below), - ch sgn(above - v); sh, sv: the exact signs of the horizontal and vertical
    differences.  Every term is an exact multiple of ONE stored coefficient c^ (|c^ - c| <= u c), so the coefficients'
    error is u (cw |kw| + ch |kh|) with kw, kh the net integer counts -- nothing where the signs cancel -- and an addition
    rounds only if its term is not 0 and the partial sum is not itself an exact multiple of that coefficient (a sum that
    started at an exact 0: k c^ with |k| <= 2 is exact)."""
    R, W = img.shape[:2]
    z = np.zeros((R, W, 2))
    right, left, down, up = z.copy(), z.copy(), z.copy(), z.copy()
    right[:sh.shape[0], :-1] = sh
    left[:sh.shape[0], 1:] = -sh
    down[:nv] = sv
    up[1:nv + 1] = -sv
    kw, kh = right + left, down + up
    same = cw == ch  # (W == H: one stored number; its multiples k c^ are exact for |k| in {0, 1, 2, 4}, not for 3)
    p, er, loose = g0.x.copy(), np.zeros_like(g0.x), np.zeros_like(g0.x)
    pure, k = g0._is0(), np.zeros_like(g0.x)
    for i, (c, sg) in enumerate(((cw, right), (cw, left), (ch, down), (ch, up))):
        if i == 2 and not same:  # from multiples of cw^ to multiples of ch^: exact only from an exact 0
            pure, k = pure & (k == 0.0), np.zeros_like(k)
        k = k + sg
        p = p + c * sg
        loose = loose + U * c * np.abs(sg)
        rounds = (sg != 0.0) & ~(pure & (np.abs(k) != 3.0))
        er = er + np.where(rounds, U * (np.abs(p) + g0.e + loose + er), 0.0)
        pure = pure & ~rounds
    coef = cw * np.abs(kw + kh) if same else cw * np.abs(kw) + ch * np.abs(kh)
    return V(p, g0.e + U * coef + er)


def tv_ref(img, R_own, W, H, weight, pre, start):
    """inr_tv_grad on img [R, W, 2] adding into ``pre`` [R, W, 2] and into a loss word that holds ``start``"""
    R = img.shape[0]
    cw, ch = tv_coeffs(weight, W, H)
    dh, dv, nv = _tv_diffs(img, R_own)
    terms = [dh.abs() * V.const(cw), dv.abs() * V.const(ch)]
    d = V.inp(pre) + _tv_accumulate(V(np.zeros(img.shape)), img, cw, ch, nv, dh.sign(), dv.sign())
    loss, lb = _word(terms, _chain(-(-(R * W * 2) // LOSS_BLOCKS), 2, False, True), start)
    return dict(loss=loss, loss_bound=lb, dout=d.x, dout_bound=d.e)


def _tv_f32(img, R_own, W, H, weight, mut=None):
    """fp32: (th, tv, parts, rest): the loss terms |d| cw and |d| ch per element, 0 where there is no pair [R, W, 2]; the
    four sign terms per element in the kernels' order; rest = (dh, dv, cw, ch, rows_h, nv) for the per-coordinate terms of
    the loss + TV kernel.  ``mut``: "swap" (cw and ch), "halo" (the halo row's horizontal pairs counted)"""
    f = np.float32
    R = img.shape[0]
    cw, ch = (f(c) for c in tv_coeffs(weight, W, H))
    if mut == "swap":
        cw, ch = ch, cw
    rows_h = R if mut == "halo" else R_own
    nv = min(R_own, R - 1)
    dh = img[:rows_h, :-1] - img[:rows_h, 1:]
    dv = img[:nv] - img[1:nv + 1]
    th, tv = np.zeros((R, W, 2), dtype=f), np.zeros((R, W, 2), dtype=f)
    th[:rows_h, :-1] = np.abs(dh) * cw
    tv[:nv] = np.abs(dv) * ch
    sh, sv = np.sign(dh), np.sign(dv)
    parts = [np.zeros((R, W, 2), dtype=f) for _ in range(4)]
    parts[0][:rows_h, :-1] = cw * sh
    parts[1][:rows_h, 1:] = -(cw * sh)
    parts[2][:nv] = ch * sv
    parts[3][1:nv + 1] = -(ch * sv)
    return th, tv, parts, (dh, dv, cw, ch, rows_h, nv)


def tv_f32(img, R_own, W, H, weight, pre, start, mut=None):
    th, tv, parts, _ = _tv_f32(img, R_own, W, H, weight, mut)
    g = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    terms = np.stack([th.reshape(-1), tv.reshape(-1)], axis=1)
    return fold32(terms, LOSS_BLOCKS, False, start=start), pre + g


def loss_tv_ref(kind, y, t, mask, count, R, R_own, W, H, weight):
    """inr_loss_tv_grad: y, t [R * W, 2]; the pointwise loss on the sampled rows r < R_own, TV as tv_ref; writes dout"""
    n = R * W
    keep = _keep(mask, n) & (np.arange(n) < R_own * W)
    ys, ts = _safe(y, t, keep)
    L, g0, g1 = (_sel(q, keep) for q in row_terms(V, kind, ys, ts, V.const(1.0 / count)))
    img = np.asarray(y, dtype=np.float32).reshape(R, W, 2)
    cw, ch = tv_coeffs(weight, W, H)
    dh, dv, nv = _tv_diffs(img, R_own)
    # per coordinate: (|d0| + |d1|) c
    ah, av = dh.abs(), dv.abs()
    terms = [L, V(ah.x.sum(axis=2), V._rd(ah.x.sum(axis=2), ah.e.sum(axis=2))) * V.const(cw),
             V(av.x.sum(axis=2), V._rd(av.x.sum(axis=2), av.e.sum(axis=2))) * V.const(ch)]
    d = V(np.stack([g0.x, g1.x], axis=1).reshape(R, W, 2), np.stack([g0.e, g1.e], axis=1).reshape(R, W, 2))
    d = _tv_accumulate(d, img, cw, ch, nv, dh.sign(), dv.sign())
    loss, lb = _word(terms, _chain(-(-n // LOSS_TV_BLOCKS), 3, True, False))
    return dict(loss=loss, loss_bound=lb, dout=d.x.reshape(n, 2), dout_bound=d.e.reshape(n, 2))


def loss_tv_f32(kind, y, t, mask, count, R, R_own, W, H, weight, mut=None):
    n = R * W
    keep = _keep(mask, n) & (np.arange(n) < R_own * W)
    ys, ts = _safe(y, t, keep)
    L, g0, g1 = (_sel(q, keep) for q in row_terms(F, kind, ys, ts, F.const(1.0 / count)))
    img = np.asarray(y, dtype=np.float32).reshape(R, W, 2)
    _, _, parts, (dh, dv, cw, ch, rows_h, nv) = _tv_f32(img, R_own, W, H, weight, mut)
    th, tv = np.zeros((R, W), dtype=np.float32), np.zeros((R, W), dtype=np.float32)
    th[:rows_h, :-1] = (np.abs(dh[..., 0]) + np.abs(dh[..., 1])) * cw
    tv[:nv] = (np.abs(dv[..., 0]) + np.abs(dv[..., 1])) * ch
    d = np.stack([g0.v, g1.v], axis=1).reshape(R, W, 2)
    for p in parts:
        d = d + p
    terms = np.stack([L.v, th.reshape(-1), tv.reshape(-1)], axis=1)
    return fold32(terms, LOSS_TV_BLOCKS, True), d.reshape(n, 2)


# ---- centre pairs ---------------------------------------------------------------------------------------------------
def pair_terms(N, y, t, ia, ib, n, weight, pre, mut=None):
    """valid pairs only: (rows a, rows b, loss terms, new dout rows of a [2], of b [2]) of class N"""
    B = len(y)
    ok = (ia >= 0) & (ia < B) & (ib >= 0) & (ib < B)
    a, b = ia[ok], ib[ok]
    w = N.const(float(np.float32(weight)) / n)
    ya, yb = [N.inp(y[a, 0]), N.inp(y[a, 1])], [N.inp(y[b, 0]), N.inp(y[b, 1])]
    mod = lambda p, q: (p * p + q * q).sqrt()
    na, nb = mod(*ya), mod(*yb)
    ta, tb = mod(N.inp(t[a, 0]), N.inp(t[a, 1])), mod(N.inp(t[b, 0]), N.inp(t[b, 1]))
    r = (ta - tb) - (na - nb)
    terms = (w * r) * r
    za, zb = na.val() > 0, nb.val() > 0  # |y| = 0 exactly iff y = (0, 0): the same rows in either class
    safe = lambda m, z: m if np.all(z) else (V(np.where(z, m.x, 1.0), np.where(z, m.e, 0.0)) if N is V else F(np.where(z, m.v, 1)))
    ca = _sel((w.times(-2.0) * r) / safe(na, za), za)
    cb = _sel((w.times(-2.0 if mut == "pair_b_sign" else 2.0) * r) / safe(nb, zb), zb)
    da = [N.inp(pre[a, o]) + ca * ya[o] for o in (0, 1)]
    db = [N.inp(pre[b, o]) + cb * yb[o] for o in (0, 1)]
    return a, b, ok, terms, da, db


def pairs_ref(y, t, ia, ib, weight, pre, start):
    """inr_center_pairs_grad adding into ``pre`` [B, 2] and into a loss word that holds ``start``"""
    n = len(ia)
    a, b, ok, terms, da, db = pair_terms(V, y, t, ia, ib, n, weight, pre)
    dout, bound = np.asarray(pre, dtype=np.float64).copy(), np.zeros(np.shape(pre))
    for o in (0, 1):
        dout[a, o], bound[a, o] = da[o].x, da[o].e
        dout[b, o], bound[b, o] = db[o].x, db[o].e
    loss, lb = _word([terms], _chain(-(-n // LOSS_BLOCKS), 1, False, True), start)
    return dict(loss=loss, loss_bound=lb, dout=dout, dout_bound=bound)


def pairs_f32(y, t, ia, ib, weight, pre, start, mut=None):
    n = len(ia)
    a, b, ok, terms, da, db = pair_terms(F, y, t, ia, ib, n, weight, pre, mut=mut)
    dout = np.array(pre, dtype=np.float32)
    for o in (0, 1):
        dout[a, o], dout[b, o] = da[o].v, db[o].v
    full = np.zeros(n, dtype=np.float32)
    full[ok] = terms.v
    return fold32(full, LOSS_BLOCKS, False, start=start), dout


# ---- comparison -----------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    """max |got - ref| / bound; a nonzero error under a zero bound, or a value that is not finite, is inf"""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    q = np.where(np.isfinite(got), q, np.inf)
    return float(q.max())


# ---- inputs ---------------------------------------------------------------------------------------------------------
_Y = (0.3, -0.2)
_f = np.float32
# (name, y, t, y for msle or None)
EDGES = (
    ("y_zero", (0.0, 0.0), (0.25, -0.125), None),                         # the denominator is eps alone
    ("y_eq_t_one", _Y, (0.3, 0.1), None),                                  # l1: sign(0) in one channel
    ("y_eq_t_both", _Y, _Y, None),                                         # ... in both (hdr: not finite, left out)
    ("zero_signs_a", (0.0, -0.0), (-0.0, 0.2), None),
    ("zero_signs_b", (-0.0, 0.3), (0.1, -0.0), None),
    ("tanh_saturated", (50.0, -47.0), (0.1, -0.2), (50.0, 47.0)),          # tanh'(y) rounds to 0
    ("diff_1e-6", _Y, (float(_f(0.3) + _f(2.5e-7)), float(_f(-0.2) - _f(2.5e-7))), None),   # |y - t| = 1e-6 |y|
    ("diff_1e3", (2e-4, -3e-4), (0.25, -0.3), None),                       # |y - t| = 1e3 |y|
    ("y_near_-1", (-1.0 + 2.0 ** -20, -1.0 + 3 * 2.0 ** -21), (0.2, -0.1), None),   # msle: y + 1 of order 1e-6
    ("hdr_lg_near_0", (0.3, 0.4), (0.3 - 0.50125, 0.4), None),             # |e| / den = 1.0005
)
NOT_FINITE = {("hdr", "y_eq_t_both")}
# Rows that may miss the usefulness cap of tests/test_loss_host.py, because the quantity is ill-conditioned in fp32 by the
# reference's own formula: NONE is needed.  The two candidates, hdr's lg = log(|e| / den) near 0 ("hdr_lg_near_0":
# lg = 5e-4 carries the roundings of a quotient at 1, about 1e-3 relative) and msle's log(y + 1 + 1e-9) of a small y
# ("y_zero", "zero_signs_a", "zero_signs_b", "diff_1e3": y + 1 rounds at 1, and 1e-9 is lost), stay inside
# 1e-2 max(|reference|, inv_count) at these inputs, so they are held to the cap like every other edge row.
ILL_CONDITIONED = frozenset()


def edge_positions(B, nblocks=LOSS_BLOCKS):
    per = -(-B // nblocks)
    last = (B - 1) // per
    pos = {0, B - 1, per - 1, last * per, 255, 256, 257}
    return sorted(p for p in pos if 0 <= p < B)


def _turn(B, sizes):
    """where the turn through EDGES starts for size B: after the positions of the sizes before it"""
    k = 0
    for b, nb in sizes:
        if b == B:
            return k
        k += len(edge_positions(b, nb))
    return k


def rows(kind, B, nblocks=LOSS_BLOCKS, sizes=None, seed=0):
    """(y, t, names): fp32 [B, 2] each and {row: edge name}"""
    sizes = [(b, LOSS_BLOCKS) for b in SIZES] if sizes is None else sizes
    if kind == "msle":
        y = np.abs(rnd(B * 2, 7 + seed, 0.3)).reshape(B, 2) + _f(0.05)
        t = np.abs(rnd(B * 2, 9 + seed, 0.3)).reshape(B, 2) + _f(0.05)
    else:
        y, t = rnd(B * 2, 8 + seed, 0.3).reshape(B, 2), rnd(B * 2, 9 + seed, 0.3).reshape(B, 2)
    names = {}
    k = _turn(B, sizes)
    for p in edge_positions(B, nblocks):
        while (kind, EDGES[k % len(EDGES)][0]) in NOT_FINITE:
            k += 1
        name, ye, te, ym = EDGES[k % len(EDGES)]
        y[p], t[p] = _f(ym if kind == "msle" and ym is not None else ye), _f(te)
        names[p] = name
        k += 1
    return y, t, names


def mask_of(tag, B, seed=10):
    """(mask uint8 [B] or None, count)"""
    if tag == "none":
        return None, B
    if tag == "half":
        m = (rnd(B, seed) > 0).astype(np.uint8)
        m[edge_positions(B)[::2]] = 1  # every other edge row stays sampled whatever the draw
        return m, max(int(m.sum()), 1)
    m = np.zeros(B, dtype=np.uint8)
    if tag == "single":
        m[B - 1] = 1
    return m, 1  # "zero": nothing sampled, count = 1


def nonfinite_rows(kind, B=300):
    """(y, t, bad): the bounded rows of ``rows`` with ONE row that is not finite in float64: hdr y == t (loss +inf,
    gradient NaN), msle y < -1 (NaN)"""
    y, t, _ = rows(kind, B, sizes=[(B, LOSS_BLOCKS)])
    bad = np.zeros(B, dtype=bool)
    bad[B // 2] = True
    if kind == "hdr":
        y[B // 2] = t[B // 2]
    elif kind == "msle":
        y[B // 2] = (_f(-1.5), _f(0.2))
    else:
        raise KeyError(kind)
    return y, t, bad


DIST_BOUNDS = ((0.1, 0.45), (-1.0, 10.0), (0.2, 0.8), (0.0, 5.0))  # pair 1 compares no row: cons_inv = 0


def multi_rows(kind, NH, B):
    """(ys [NH, B, 2], t, dist [B]): head k is ``rows`` with another seed; dist in [0, 1), and on the rows next to the
    edge positions (where the heads differ: on the edge rows themselves every head holds the same y) exactly lo and hi
    of pair 0 and one fp32 step outside each, in turn"""
    t = rows(kind, B)[1]
    ys = np.stack([rows(kind, B, seed=20 + k)[0] for k in range(NH)])
    dist = np.abs(rnd(B, 11, 1.0))
    lo, hi = _f(DIST_BOUNDS[0][0]), _f(DIST_BOUNDS[0][1])
    vals = (lo, hi, np.nextafter(lo, _f(-1)), np.nextafter(hi, _f(2)))
    pos = edge_positions(B)
    near = []
    for step in (1, -1, 2, -2):
        near += [q + step for q in pos if 0 <= q + step < B and q + step not in pos and q + step not in near]
    for k, p in enumerate(near):
        dist[p] = vals[k % 4]
    return ys, t, dist


def tv_rows(kind, R, R_own, W):
    """(y, t) [R * W, 2]: ``rows`` over the 256 blocks of the loss + TV kernel, with equal neighbours (sign 0) and
    +-0.0 next to each other in the image"""
    n = R * W
    y, t, names = rows(kind, n, LOSS_TV_BLOCKS, sizes=[(r * w, LOSS_TV_BLOCKS) for r, _, w, _ in TV_SHAPES])
    img = y.reshape(R, W, 2)
    if n > 4:
        img[0, 1] = img[0, 0]                 # horizontal pair with d = 0 in both channels
        img[R - 1, W - 1] = img[R - 2, W - 1]  # vertical pair with d = 0 (the halo row's, where there is one)
    if R >= 3 and W >= 3:
        img[1, W - 3] = (_f(0.0), _f(-0.0))
        img[1, W - 2] = (_f(-0.0), _f(0.0))
    return y, t, names


def pair_rows(n, B=PAIR_B):
    """(y, t, ia, ib): a rows distinct in [0, B / 2), b rows distinct in [B / 2, B), as the entry demands (it updates dout
    without atomics); a pair row at the origin; from n >= 64 on one index of -1 and one of B.  B rows hold at most B / 2
    such pairs: of the 16385 the pairs from B / 2 on have an index outside [0, B) in turn (-1 in a, B in b, 10^9 in a), so
    blocks 0 .. 38 of the 64 (257 pairs each, a second trip for lane 0) do work and the rest add nothing."""
    y, t = rnd(B * 2, 17, 0.3).reshape(B, 2), rnd(B * 2, 18, 0.3).reshape(B, 2)
    i = np.arange(n, dtype=np.int64)
    half = B // 2
    ia, ib = (i * 7919) % half, half + (i * 7907) % half  # both multipliers are prime to B / 2 = 10000
    out = i >= half
    ia[out & (i % 3 == 0)], ib[out & (i % 3 == 1)], ia[out & (i % 3 == 2)] = -1, B, 10 ** 9
    m = min(n, half)
    assert len(set(ia[:m])) == m and len(set(ib[:m])) == m
    y[ia[0]] = (_f(0.0), _f(0.0))
    if n > 2:
        y[ib[m - 1]] = (_f(0.0), _f(-0.0))
    if n >= 64:
        ia[5], ib[m - 2] = -1, B
    return y, t, ia, ib


# ---- the same rows through the fused kernels ------------------------------------------------------------------------
FUSED_B = 129
FUSED_OUT = ((0.0, 0.0), (0.3, -0.2))


def fused_targets(kind, b, B=FUSED_B):
    """t [B, 2] for a network whose every output row is y = b: closed-form fill, then targets that put the rows 0, 1, ...
    and the rows 127, 128 (the last of the first 128-row tile, the first of the next) on an edge in turn"""
    b = np.asarray(b, dtype=np.float32)
    t = rnd(B * 2, 9, 0.3).reshape(B, 2)
    if kind == "msle":
        t = np.abs(t) + _f(0.05)
    den = float(np.sqrt(float(b[0]) ** 2 + float(b[1]) ** 2)) + EPS
    tiny = b * _f(1.0 + 2.0 ** -20) if b.any() else np.array([3e-7, -2e-7], dtype=np.float32)
    far = b * _f(1e3) if b.any() else np.array([50.0, -47.0], dtype=np.float32)
    edges = [b.copy(), np.array([b[0], 0.1], dtype=np.float32), np.array([0.0, -0.0], dtype=np.float32),
             np.array([-0.0, 0.2], dtype=np.float32), tiny, far, np.array([b[0] - _f(den * 1.0005), b[1]], dtype=np.float32)]
    if kind == "hdr":
        edges = edges[1:] if b.any() else [e for e in edges[1:] if e.any()]  # y == t: not finite (loss_cases.NOT_FINITE)
    if kind == "msle":
        edges = [np.abs(e) for e in edges]
    pos = list(range(len(edges))) + [127, 128]
    for k, p in enumerate(pos):
        t[p] = edges[k % len(edges)]
    return t


def fused_ref(kind, b, t, hdr_A=HDR_A):
    """loss word and last-layer bias gradient (sum over rows of g) of a fused step whose output is y = b on every row:
    dict(loss, loss_bound, bias [2], bias_bound [2]).  Whatever tree the kernel and the slab reduction add the B row terms
    in (padding adds exact zeros), no chain is longer than B - 1 additions"""
    B = len(t)
    y = np.tile(np.asarray(b, dtype=np.float32), (B, 1))
    L, g0, g1 = row_terms(V, kind, y, t, V.const(1.0 / B), hdr_A=hdr_A)
    loss, lb = _word([L], B - 1)
    bias = [_word([g], B - 1) for g in (g0, g1)]
    return dict(loss=loss, loss_bound=lb, bias=np.array([bias[0][0], bias[1][0]]), bias_bound=np.array([bias[0][1], bias[1][1]]))
