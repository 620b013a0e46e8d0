"""Cases and references of tests/test_focal_host.py (CPU) and tests/test_gpu_focal.py: the arithmetic of
inr_focal_loss_grad (csrc/inr_loss_focal.hip) against a float64 statement, element by element.  A plain
module like loss_cases.py, whose number classes and rules it uses: the formula is written ONCE (``focal_terms``) over ``V``
(the float64 value with a bound on |fp32 result - value|) and over ``F`` (the fp32 restatement).

Per sampled row, in the kernel's order (include/inr_abi.h):
    e_o = y_o - t_o;  q = e_0 e_0 + e_1 e_1;  m = sqrt(q) or pow(sqrt(q), alpha);  n = log(m + 1) or m
    n_max = max n;  w = clamp(n / n_max, 0, 1) or 0 when n_max == 0;  term = w q
    loss = ((sum term) inv) lw;  dout_o = (((lw 2) e_o) w) inv

Two rules beyond loss_cases.py's, both inequalities:
    pow   f(x) = x^alpha of x >= 0 known to e_x, alpha an exact fp32 constant > 0, in the form of the log rule:
              e' = sup|f'| e_x + K_POW u (|f(x)| + sup|f'| e_x),   f' = alpha x^(alpha - 1), its sup over [x - e_x, x + e_x]
              taken at x + e_x for alpha >= 1 and at x - e_x (which must be > 0) for alpha < 1;  pow(0, alpha) of an exact 0
              is an exact 0.  K_POW = 4: as for K_LOG, it is meant to be twice the max-ulp figure of HIP's math documentation
              for powf; a ROCm installation ships no such table, so the same fallback value 4 is used.
    n_max the computed maximum of computed values n^_r with |n^_r - n_r| <= b_r lies within max_r b_r of max_r n_r (a max is
              1-Lipschitz in the sup norm; it adds no rounding of its own).  That bound enters w through V's division rule;
              the clamp to [0, 1] is 1-Lipschitz and the exact w lies in [0, 1], so it adds nothing.
The loss word: loss_cases._word with the chain of this kernel -- a lane's 2 ceil(per / 256) terms (per = pairs per block), 8
tree levels, the 255 partials in order -- then the two products by V's rule.  Nothing is fitted to what a device returns.
"""
import numpy as np

import loss_cases as C
from aux_bits_cases import rnd
from loss_cases import F, V

K_POW = 4  # no ulp table installed: the fallback value (module docstring)
BLOCKS = 255  # INR_FOCAL_BLOCKS
SIZES = (1, 2, 255, 256, 257, 513, 1000, 65537)
COMBOS = tuple((a, lg) for a in (1.0, 0.5, 2.0) for lg in (True, False))
BIG = (np.float32(1.0), np.float32(-1.0))  # |e| = 1.41 against at most 0.85 of the amplitude-0.3 rows


# ---- the two rules ----------------------------------------------------------------------------------------------------
def vpow(a, alpha):
    assert float(np.float32(alpha)) == float(alpha) and alpha > 0.0
    zero = a._is0()
    xs = np.where(zero, 1.0, a.x)
    lo = xs - a.e
    if alpha < 1.0:
        assert np.all(lo > 0.0), "pow with alpha < 1 of a value that may be 0"
        slope = alpha * lo ** (alpha - 1.0)
    else:
        slope = alpha * (xs + a.e) ** (alpha - 1.0)
    x = xs ** alpha
    C._normal(x)
    r = V(x, V._rd(x, slope * a.e, K_POW))
    return V(np.where(zero, 0.0, r.x), np.where(zero, 0.0, r.e))


def fpow(a, alpha):
    with np.errstate(all="ignore"):
        return F(np.power(a.v.astype(np.float64), np.float64(np.float32(alpha))).astype(np.float32))


def vmax(n, live):
    """(V of n_max, index of a row that attains it) over the live rows; an exact 0 when there are none"""
    if not live.any():
        return V(0.0), None
    idx = np.flatnonzero(live)
    k = idx[int(np.argmax(n.x[idx]))]
    return V(n.x[k], float(n.e[idx].max())), int(k)


# ---- the formula, once ------------------------------------------------------------------------------------------------
def focal_terms(N, y, t, live, alpha, log_matrix, lw, inv):
    """(term [B], d0 [B], d1 [B], n_max) of class N; rows that are not live are exact zeros.  lw, inv: N constants"""
    y, t = np.asarray(y, dtype=np.float32), np.asarray(t, dtype=np.float32)
    E = [N.inp(y[:, o]) - N.inp(t[:, o]) for o in (0, 1)]
    q = E[0] * E[0] + E[1] * E[1]
    m = q.sqrt()
    if alpha != 1.0:
        m = vpow(m, alpha) if N is V else fpow(m, alpha)
    n = (m + N.exact(1.0)).log() if log_matrix else m
    if N is V:
        n_max, _ = vmax(n, live)
        none = float(n_max.x) == 0.0
        w = V(np.zeros(len(y))) if none else n / V(np.full(len(y), float(n_max.x)), np.full(len(y), float(n_max.e)))
        if not none:
            assert np.all((w.x[live] >= 0.0) & (w.x[live] <= 1.0))  # the clamp changes no exact value of a sampled row
    else:
        nm = np.float32(n.v[live].max()) if live.any() else np.float32(0)
        n_max = F(nm)
        with np.errstate(all="ignore"):
            w = F(np.zeros(len(y))) if nm == 0 else F(np.minimum(np.maximum(n.v / nm, np.float32(0)), np.float32(1)))
    lw2 = lw.times(2.0)
    term = C._sel(w * q, live)
    d = [C._sel(((lw2 * E[o]) * w) * inv, live) for o in (0, 1)]
    return term, d[0], d[1], n_max


def chain(B):
    pairs = (B + 1) // 2
    per = -(-pairs // BLOCKS)
    return 2 * -(-per // 256) + 8 + BLOCKS


def focal_ref(y, t, mask, count, alpha=1.0, log_matrix=True, lw=1.0):
    """dict(loss, loss_bound, dout [B,2], dout_bound, n_max, n_max_bound): float64 values and bounds on the kernel's error"""
    B = len(y)
    live = C._keep(mask, B)
    term, d0, d1, n_max = focal_terms(V, y, t, live, alpha, log_matrix, V.const(lw), V.const(1.0 / count))
    s, sb = C._word([term], chain(B))
    loss = (V(s, sb) * V.const(1.0 / count)) * V.const(lw)
    return dict(loss=float(loss.x), loss_bound=float(loss.e), dout=np.stack([d0.x, d1.x], axis=1),
                dout_bound=np.stack([d0.e, d1.e], axis=1), n_max=float(n_max.x), n_max_bound=float(n_max.e))


def focal_f32(y, t, mask, count, alpha=1.0, log_matrix=True, lw=1.0):
    """the fp32 restatement over F: (per-row terms [B], dout [B,2], n_max) -- the sum of the terms is the kernel's fold
    (inr_mi355x.focal._fold32)"""
    live = C._keep(mask, len(y))
    term, d0, d1, n_max = focal_terms(F, y, t, live, alpha, log_matrix, F.const(lw), F.const(1.0 / count))
    return term.v, np.stack([d0.v, d1.v], axis=1), n_max.v


# ---- inputs -----------------------------------------------------------------------------------------------------------
def block_rows(B):
    """rows [lo, hi) of the non-empty blocks: block b takes the pairs [b per, (b + 1) per)"""
    pairs = (B + 1) // 2
    per = -(-pairs // BLOCKS)
    last = (pairs - 1) // per
    return [(2 * b * per, min(2 * (b + 1) * per, B)) for b in range(last + 1)]


def max_positions(B):
    """row 0, row B - 1, first and last row of the first and of the last non-empty block"""
    blocks = block_rows(B)
    pos = {0, B - 1, blocks[0][0], blocks[0][1] - 1, blocks[-1][0], blocks[-1][1] - 1}
    return sorted(pos)


def rows(B, seed=0):
    """y, t fp32 [B,2] at amplitude 0.3"""
    return rnd(B * 2, 61 + seed, 0.3).reshape(B, 2), rnd(B * 2, 62 + seed, 0.3).reshape(B, 2)


def with_max_at(y, t, p):
    y = y.copy()
    y[p] = (t[p, 0] + BIG[0], t[p, 1] + BIG[1])
    return y


def random_mask(B, seed=63):
    m = (rnd(B, seed) > 0).astype(np.uint8)
    return m
