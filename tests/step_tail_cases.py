"""Cases and references of tests/test_step_tail_host.py (CPU) and tests/test_gpu_step_tail.py: the tail of every training
step (csrc/inr_params.hip -- slab reduction, Adam update fused with the re-pack of the weight images, sharded update)
against plain numpy statements of what it computes.  A plain module like aux_bits_cases.py, not a conftest.

The references
--------------
``adam_ref64``  torch.optim.Adam's single-tensor algorithm (amsgrad=False) in float64 from the fp32 inputs, with the
    penalty terms of include/inr_abi.h (inr_adam_step), every hyper-parameter a Python double:
        1. g += wd * p                     2. g += l1 * sign(p), sign(+-0) = 0        3. g += 2 * l2 * p
        4. m += (1 - b1) * (g - m)         5. v = b2 * v + (1 - b2) * g * g
        6. denom = sqrt(v) / sqrt(1 - b2^t) + eps          7. p -= lr / (1 - b1^t) * m / denom
    Entries with live == False keep p, m and v.  tests/test_step_tail_host.py anchors it to torch.optim.Adam in float64.

``adam_f32``  the same seven steps with every operation rounded to fp32 (numpy), constants stored as fp32, and the three
    places where the header's arithmetic is a fused multiply-add (steps 1, 3 and the last operation of 5) rounded once.
    It is what an fp32 implementation of the contract computes; the CPU module holds it to ``adam_bound``.

``adam_bound``  a per-entry bound on |fp32 result - adam_ref64| for p, m and v, by forward error analysis.  u = 2^-24.
    An exact quantity X is carried with a bound e on |computed - X|; the rules are
        constant c stored as fp32:         e = u |c|        (wd, l1, 2 * l2, 1 - b1, b2, 1 - b2, eps, and the two table
                                                             values step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t))
        rounding of a result X:            e' = e + k u (|X| + e)      k = 1 for + - * fma;  k = 2 for sqrt and / (HIP
                                                             documents 1 ulp for both; IEEE numpy gives k = 1)
        a + b:                             e = ea + eb
        a * b:                             e = |a| eb + |b| ea + ea eb
        a / b:                             e = (ea + |a / b| eb) / (|b| - eb)
        sqrt(a):                           e = min(ea / sqrt(a), sqrt(ea))      (|sqrt x - sqrt y| <= sqrt |x - y|)
    applied in the order of the update:
        g1 = round(g + wd p)  [fma]        g2 = round(g1 + l1 sign p)           g3 = round(g2 + (2 l2) p)  [fma]
        d = round(g3 - m),  w = round(d (1 - b1)),  m' = round(m + w)
        q = round(g3 g3),  r = round(v b2),  v' = round(q (1 - b2) + r)  [fma]
        s = round2(sqrt v'),  x = round2(s / bc2_sqrt),  den = round(x + eps)
        t = round2(m' / den),  up = round(step_size t),  p' = round(p - up)
    A step that is skipped (wd, l1 or l2 == 0) adds nothing.  Where a compiler contracts one of the two-rounding pairs
    (w and m', l1 and g2, up and p') into an fma the error only shrinks: |fma error| <= the second rounding alone.  Nothing
    is neglected to first order or fitted: every rule above is an inequality.  At g == m == v == 0 (and no penalty) every
    term is 0 and the bound demands the exact result: p unchanged, moments 0.

    The rounding rule e' = e + u |X| holds in the fp32 NORMAL range only, so every input set keeps every product and
    quotient above either exactly 0 or above 2^-120 in magnitude, and far below overflow; ``adam_bound`` asserts it
    (sums and differences are exact when they fall below the normal range).  Nothing here relies on overflow or denormal
    behaviour.

``flat_sum_ref32``  the summation tree of flat_slab_sum in numpy fp32, for bit-equality: the n slabs in four contiguous
    quarters of per = ceil(n / 4), each quarter added in slab order from +0 (the 8-deep batches change the loads, not the
    order), combined as ((q0 + q1) + q2) + q3.  ``flat_sum_ref64``: the float64 sum and the textbook bound
    (n - 1) 2^-24 sum |terms| of fp32 summation (the tree's longest chain is at most n - 1 additions).

Edge inputs (``edge_state``): vectors filled from aux_bits_cases.rnd, then overwritten at the first and last entry of
every tensor (weights and bias of every layer), at entries 255, 256, 257 and at P - 1 with the rows of EDGES in turn.
"""
import numpy as np

from aux_bits_cases import rnd

U = 2.0 ** -24
TINY = 2.0 ** -120

STEPS = (1, 2, 1000)
HYPER = ((0.0, 0.0, 0.0), (1e-4, 0.0, 0.0), (0.0, 1e-6, 0.0), (0.0, 0.0, 1e-5), (1e-4, 1e-6, 1e-5))  # (wd, l1, l2)
HYPER_COMPLEX = HYPER[:2]  # plans with complex64 tensors: the Adam entries refuse l1 / l2
BETAS = (0.9, 0.999)
BETAS_ONCE = (0.8, 0.99)
LR, EPS = 1e-3, 1e-8


# ---- Adam -----------------------------------------------------------------------------------------------------------
def _f64(*a):
    return [np.asarray(x, dtype=np.float64).copy() for x in a]


def adam_ref64(p, g, m, v, step, lr, b1, b2, eps, wd, l1, l2, live=None):
    """(p, m, v) after one update, float64; ``live`` (bool array or None): False entries are returned unchanged"""
    p0, g, m0, v0 = _f64(p, g, m, v)
    g = g + wd * p0
    g = g + l1 * np.sign(p0)  # numpy: sign(+-0) = 0
    g = g + 2.0 * l2 * p0
    m1 = m0 + (1.0 - b1) * (g - m0)
    v1 = b2 * v0 + (1.0 - b2) * g * g
    denom = np.sqrt(v1) / np.sqrt(1.0 - b2 ** step) + eps
    p1 = p0 - lr / (1.0 - b1 ** step) * m1 / denom
    if live is not None:
        p1, m1, v1 = np.where(live, p1, p0), np.where(live, m1, m0), np.where(live, v1, v0)
    return p1, m1, v1


def _fma32(a, b, c):
    """round(a * b + c) to fp32 through float64: the product of two fp32 is exact there (the one extra rounding of the
    sum to 53 bits moves an fp32 result in fewer than one case in 2^28)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam_f32(p, g, m, v, step, lr, b1, b2, eps, wd, l1, l2, live=None):
    """the seven steps with fp32 arithmetic and fp32 constants (see the module docstring); returns fp32 (p, m, v)"""
    f = np.float32
    p0, g, m0, v0 = (np.asarray(x, dtype=f).copy() for x in (p, g, m, v))
    step_size, bc2_sqrt = f(lr / (1.0 - b1 ** step)), f(np.sqrt(1.0 - b2 ** step))
    if wd != 0.0:
        g = _fma32(f(wd), p0, g)
    if l1 != 0.0:
        g = g + f(l1) * np.sign(p0).astype(f)
    if l2 != 0.0:
        g = _fma32(f(2.0) * f(l2), p0, g)
    m1 = m0 + (g - m0) * f(1.0 - b1)
    v1 = _fma32(g * g, f(1.0 - b2), v0 * f(b2))
    denom = np.sqrt(v1) / bc2_sqrt + f(eps)
    p1 = p0 - step_size * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == f
    if live is not None:
        p1, m1, v1 = np.where(live, p1, p0), np.where(live, m1, m0), np.where(live, v1, v0)
    return p1, m1, v1


def _normal(*xs):
    for x in xs:
        a = np.abs(x)
        assert np.all((a == 0.0) | ((a > TINY) & (a < 2.0 ** 100))), "an intermediate leaves the fp32 normal range"


def adam_bound(p, g, m, v, step, lr, b1, b2, eps, wd, l1, l2, live=None):
    """(ep, em, ev): per-entry bounds on |fp32 - adam_ref64| of params, exp_avg, exp_avg_sq (module docstring)"""
    p, G, m, v = _f64(p, g, m, v)
    u = U

    def rd(x, e, k=1):
        return e + k * u * (np.abs(x) + e)

    eG = np.zeros_like(G)
    if wd != 0.0:
        t = wd * p
        _normal(t)
        G, eG = G + t, rd(G + t, eG + u * np.abs(t))
    if l1 != 0.0:
        s = l1 * np.sign(p)
        G, eG = G + s, rd(G + s, eG + u * np.abs(s))
    if l2 != 0.0:
        t = 2.0 * l2 * p
        _normal(t)
        G, eG = G + t, rd(G + t, eG + u * np.abs(t))
    w1, w2 = 1.0 - b1, 1.0 - b2
    D = G - m
    eD = rd(D, eG)
    W = D * w1
    eW = rd(W, np.abs(D) * u * w1 + eD * w1 * (1.0 + u))
    M = m + W
    eM = rd(M, eW)
    Q = G * G
    eQ = rd(Q, 2.0 * np.abs(G) * eG + eG * eG)
    R = v * b2
    eR = rd(R, u * np.abs(R))
    V = Q * w2 + R
    eV = rd(V, eQ * w2 * (1.0 + u) + np.abs(Q) * u * w2 + eR)
    S = np.sqrt(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        eS = np.where(V > 0.0, np.minimum(eV / S, np.sqrt(eV)), np.sqrt(eV))
    eS = rd(S, eS, 2)
    bc = np.sqrt(1.0 - b2 ** step)
    ebc = u * bc
    X = S / bc
    eX = rd(X, (eS + np.abs(X) * ebc) / (bc - ebc), 2)
    Dn = X + eps
    eDn = rd(Dn, eX + u * eps)
    assert np.all(Dn > 2.0 * eDn)
    T = M / Dn
    eT = rd(T, (eM + np.abs(T) * eDn) / (Dn - eDn), 2)
    ss = lr / (1.0 - b1 ** step)
    Up = ss * T
    eUp = rd(Up, ss * (1.0 + u) * eT + u * ss * np.abs(T))
    eP = rd(p - Up, eUp)
    _normal(W, Q, Q * w2, R, X, T, Up)
    if live is not None:
        eP, eM, eV = np.where(live, eP, 0.0), np.where(live, eM, 0.0), np.where(live, eV, 0.0)
    return eP, eM, eV


def worst_ratio(got, ref, bound):
    """max over entries and over (p, m, v) of |got - ref| / bound; a nonzero error under a zero bound is inf"""
    worst = 0.0
    for a, r, b in zip(got, ref, bound):
        err = np.abs(np.asarray(a, dtype=np.float64) - r)
        assert np.all(np.isfinite(err))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / b)
        worst = max(worst, float(q.max()))
    return worst


# ---- edge inputs ----------------------------------------------------------------------------------------------------
# (p, g, m, v); None keeps the closed-form fill.  |g| and |p| from 1e-12 to 1e3 with both signs; the zeros of the issue.
EDGES = (
    (+0.0, None, None, None),          # sign(+0) = 0 under l1
    (-0.0, None, None, None),          # sign(-0) = 0
    (None, 0.0, 0.0, 0.0),             # 0 / eps (with a penalty: the penalty's gradient alone)
    (None, 0.0, None, None),           # g = 0 with old moments
    (1e-12, -1e3, None, None),
    (-1e3, 1e-12, None, None),
    (1e-8, 1e-4, None, None),
    (-1e-4, -1e-8, None, None),
    (1.0, 1.0, None, None),
    (-1.0, 1e3, None, None),
    (1e3, -1e-12, 0.0, 0.0),
    (-1e-12, 1e-12, 0.0, 0.0),
    (-0.0, -1e-12, None, None),
    (+0.0, 0.0, 0.0, 0.0),             # everything zero: no penalty can move it either
)


def edge_positions(P, tensors):
    """sorted positions: first and last entry of every tensor (offset, count), 255, 256, 257, P - 1"""
    pos = {255, 256, 257, P - 1}
    for off, n in tensors:
        pos.update((off, off + n - 1))
    return sorted(q for q in pos if 0 <= q < P)


def edge_state(P, tensors):
    """fp32 (p, g, m, v) of P entries: closed-form fill, EDGES in turn at edge_positions"""
    p, g = rnd(P, 1, 0.1), rnd(P, 5, 1e-2)
    m, v = rnd(P, 6, 1e-2), np.abs(rnd(P, 7, 1e-4))
    pos = edge_positions(P, tensors)
    assert len(pos) >= len(EDGES)
    for k, q in enumerate(pos):
        for arr, val in zip((p, g, m, v), EDGES[k % len(EDGES)]):
            if val is not None:
                arr[q] = np.float32(val)
    return p, g, m, v


def tensors_of(plan):
    """[(offset, count)] of the parameter tensors of an aux_bits_cases._engine plan, in flat (state_dict) order: from the
    package's own model classes (their _layout), built on the CPU"""
    import inr_mi355x as M
    from inr_mi355x import mfn
    wire = dict(network_input_size=3, network_output_size=2, network_depth=2, first_omega_0=10, hidden_omega_0=10, scale=5)
    model = {
        "siren32": lambda: M.SIREN(dict(network_input_size=16, network_output_size=2, network_depth=4, network_width=32)),
        "siren256": lambda: M.SIREN(dict(network_input_size=512, network_output_size=2, network_depth=5, network_width=256)),
        "wire": lambda: M.WIRE(dict(wire, network_width=46)),  # int(46 / sqrt 2) = the plan's 32 complex features
        "wire2d": lambda: M.WIRE2D(dict(wire, network_width=32)),
        "gabor": lambda: mfn.GaborNet(dict(network_input_size=16, network_output_size=2, network_depth=3, network_width=32)),
    }[{"siren32_by_image": "siren32", "siren256_bf16": "siren256"}.get(plan, plan)]()
    return [(int(o), int(n)) for (o, n, _, _) in model._layout]


MS_WIDTH, MS_ENC = 20, 8


def multiscale(depth):
    """(engine, tensors, live mask [P]) of a MultiscaleKFourier plan made as tests/matrix_cases.py makes it; the heads
    past the last output stage, the stages behind it and the heads between output stages are dead (mfn.py: _live)"""
    from inr_mi355x import _lib as L
    from inr_mi355x import mfn
    from inr_mi355x.engine import MFNEngine
    net = dict(network_input_size=2 * MS_ENC, network_output_size=2, network_depth=depth, network_width=MS_WIDTH)
    model = mfn.MultiscaleKFourier(net)
    eng = MFNEngine(L.KIND_MSFOURIER, 2 * MS_ENC, MS_WIDTH, depth, 2, MS_ENC)
    tensors = [(int(o), int(n)) for (o, n, _, _) in model._layout]
    live = np.zeros(eng.n_params, dtype=bool)
    for (o, n), lv in zip(tensors, model._live):
        live[o:o + n] = lv
    return eng, tensors, live


def dead_ranges(tensors, live):
    """the dead tensors merged into maximal [lo, hi) runs of the flat vector"""
    runs = []
    for o, n in sorted(tensors):
        if not live[o]:
            if runs and runs[-1][1] == o:
                runs[-1][1] = o + n
            else:
                runs.append([o, o + n])
    return runs


# ---- slab reduction -------------------------------------------------------------------------------------------------
def flat_sum_ref32(slabs, n=None, per=None):
    """flat_slab_sum's tree on slabs [n, P] (fp32): quarters of ``per`` slabs (default ceil(n / 4)), each added in slab
    order from +0, then ((q0 + q1) + q2) + q3"""
    slabs = np.asarray(slabs, dtype=np.float32)
    n = slabs.shape[0] if n is None else n
    per = (n + 3) // 4 if per is None else per
    q = []
    for w in range(4):
        s = np.zeros(slabs.shape[1], dtype=np.float32)
        for b in range(w * per, min(w * per + per, n)):
            s = s + slabs[b]
        q.append(s)
    out = ((q[0] + q[1]) + q[2]) + q[3]
    assert out.dtype == np.float32
    return out


def flat_sum_ref64(slabs):
    """(float64 sum over slabs, the textbook bound (n - 1) 2^-24 sum |terms|)"""
    s = np.asarray(slabs, dtype=np.float64)
    n = s.shape[0]
    return s.sum(axis=0), (n - 1) * U * np.abs(s).sum(axis=0)


SLAB_COUNTS = ("1", "2", "3", "4", "5", "9", "33+")
