"""The references of tests/step_tail_cases.py, checked without a GPU: adam_ref64 against torch.optim.Adam in float64;
the derivation of adam_bound against an fp32 restatement of the update on every edge input; flat_sum_ref32 against a
naive per-quarter loop.  tests/test_gpu_step_tail.py holds the kernels to the same references."""
import numpy as np
import pytest
import torch

import step_tail_cases as S
from aux_bits_cases import rnd


def test_adam_ref64_is_torch_adam_in_float64():
    """five steps of torch.optim.Adam (float64, single-tensor, weight_decay != 0) from zero moments; adam_ref64 is fed
    its own state back.  The two differ in the association of step 7 alone (torch: addcdiv(m, denom, -step_size)), a few
    roundings of the update per step: 64 ulp of float64 on every quantity."""
    n, lr, b1, b2, eps, wd = 37, 1e-3, 0.9, 0.999, 1e-8, 1e-4
    p0 = rnd(n, 1, 0.1).astype(np.float64)
    p0[:2] = (0.0, -0.0)
    t = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([t], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=False, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = rnd(n, 10 + step, 1e-2).astype(np.float64)
        g[3] = 0.0
        t.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = S.adam_ref64(p, g, m, v, step, lr, b1, b2, eps, wd, 0.0, 0.0)
        st = opt.state[t]
        for name, got, want in (("p", p, t.detach().numpy()), ("m", m, st["exp_avg"].numpy()),
                                ("v", v, st["exp_avg_sq"].numpy())):
            err = np.abs(got - want)
            assert np.all(err <= 64 * 2.0 ** -53 * np.abs(want)), (step, name, float(err.max()))


def test_adam_ref64_penalties_and_dead_entries():
    """the three penalty terms by hand on one entry each, sign(+-0) = 0, and live == False"""
    p = np.array([0.5, -0.5, 0.0, -0.0, 0.25], dtype=np.float32)
    g = np.zeros(5, dtype=np.float32)
    z = np.zeros(5)
    for wd, l1, l2, geff in ((0.1, 0, 0, 0.1 * p.astype(np.float64)), (0, 0.1, 0, np.array([0.1, -0.1, 0, 0, 0.1])),
                             (0, 0, 0.1, 0.2 * p.astype(np.float64))):
        _, m, v = S.adam_ref64(p, g, z, z, 1, 1e-3, 0.9, 0.999, 1e-8, wd, l1, l2)
        assert np.allclose(m, (1 - 0.9) * geff, rtol=1e-15, atol=0) and np.allclose(v, (1 - 0.999) * geff ** 2, rtol=1e-14, atol=0)
    live = np.array([True, False, True, False, True])
    p1, m1, v1 = S.adam_ref64(p, g + 1, z + 2, z + 3, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.1, live)
    assert np.array_equal(p1[~live], p[~live]) and np.all(m1[~live] == 2) and np.all(v1[~live] == 3)
    assert np.all(p1[live] != p[live])
    b = S.adam_bound(p, g + 1, z + 2, z + 3, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.1, live)
    assert all(np.all(e[~live] == 0) and np.all(e[live] > 0) for e in b)


def _edge_sets():
    """(name, P, tensors): the layouts of the GPU module's plans, and a tiny one"""
    yield "tiny", 300, [(0, 64), (64, 8), (72, 56), (128, 8), (136, 96), (232, 12), (244, 52), (296, 4)]
    for plan in ("siren32", "wire", "wire2d", "gabor"):
        t = S.tensors_of(plan)
        yield plan, t[-1][0] + t[-1][1], t
    for depth in (2, 8):
        _, t, _ = S.multiscale(depth)
        yield f"multiscale{depth}", max(o + n for o, n in t), t


def test_edge_state_holds_every_edge():
    p, g, m, v = S.edge_state(2722, S.tensors_of("siren32"))
    pos = S.edge_positions(2722, S.tensors_of("siren32"))
    assert {0, 511, 512, 543, 255, 256, 257, 2656, 2719, 2720, 2721} <= set(pos)
    at = lambda a: a[pos]
    assert np.any((at(p) == 0) & ~np.signbit(at(p))) and np.any((at(p) == 0) & np.signbit(at(p)))
    assert np.any((at(g) == 0) & (at(m) == 0) & (at(v) == 0)) and np.any((at(g) == 0) & (at(m) != 0) & (at(v) != 0))
    for a in (at(p), at(g)):
        assert a.min() <= -1e3 and a.max() >= 1e3 and 0 < np.abs(a[a != 0]).min() <= 1e-12
    assert all(np.all(np.isfinite(a)) for a in (p, g, m, v)) and np.all(v >= 0)


@pytest.mark.parametrize("name,P,tensors", list(_edge_sets()), ids=lambda a: a if isinstance(a, str) else None)
def test_fp32_restatement_within_adam_bound(name, P, tensors):
    """If this fails the derivation in step_tail_cases.py's docstring is wrong: correct the analysis."""
    p, g, m, v = S.edge_state(P, tensors)
    worst = 0.0
    combos = [(s, h, S.BETAS) for s in S.STEPS for h in S.HYPER] + [(2, S.HYPER[-1], S.BETAS_ONCE)]
    for step, (wd, l1, l2), (b1, b2) in combos:
        args = (p, g, m, v, step, S.LR, b1, b2, S.EPS, wd, l1, l2)
        ref, got, bound = S.adam_ref64(*args), S.adam_f32(*args), S.adam_bound(*args)
        r = S.worst_ratio(got, ref, bound)
        assert r <= 1.0, (name, step, wd, l1, l2, b1, r)
        worst = max(worst, r)
        # the bound stays a rounding-error bound: a few dozen roundings of the quantities involved, not a tolerance
        scale = np.abs(ref[0]) + np.abs(np.asarray(p, dtype=np.float64) - ref[0])
        assert np.all(bound[0] <= 64 * S.U * scale + 1e-300)
    print(f"{name}: worst |adam_f32 - adam_ref64| / adam_bound = {worst:.3f}")
    assert worst > 0.01  # ... and is not slack by orders of magnitude


def test_adam_bound_rejects_the_mutations():
    """the four slips of the issue's mutation list that live in the update's arithmetic, restated in fp32: each leaves the bound somewhere on
    the edge inputs (reference side of the mutation check; the kernel side needs the GPU)"""
    f = np.float32
    tensors = S.tensors_of("siren32")
    p, g, m, v = S.edge_state(2722, tensors)
    b1, b2 = S.BETAS

    def ratio(got, step, wd, l1, l2):
        args = (p, g, m, v, step, S.LR, b1, b2, S.EPS, wd, l1, l2)
        return S.worst_ratio(got, S.adam_ref64(*args), S.adam_bound(*args))

    # eps inside the square root
    v1 = S._fma32(g * g, f(1 - b2), v * f(b2))
    m1 = m + (g - m) * f(1 - b1)
    bad = p - f(S.LR / (1 - b1)) * (m1 / np.sqrt(v1 / f(1 - b2) + f(S.EPS)))
    assert ratio((bad, m1, v1), 1, 0, 0, 0) > 1
    # bc2_sqrt of step t - 1
    bad = p - f(S.LR / (1 - b1 ** 2)) * (m1 / (np.sqrt(v1) / f(np.sqrt(1 - b2 ** 1)) + f(S.EPS)))
    assert ratio((bad, m1, v1), 2, 0, 0, 0) > 1
    # l1 with p >= 0
    g1 = g + f(1e-6) * np.where(p >= 0, f(1), f(-1))
    pm, mm, vm = S.adam_f32(p, g1, m, v, 1, S.LR, b1, b2, S.EPS, 0, 0, 0)
    assert ratio((pm, mm, vm), 1, 0, 1e-6, 0) > 1
    # weight decay on dead entries
    live = np.arange(2722) >= 544
    got = S.adam_f32(p, g, m, v, 1, S.LR, b1, b2, S.EPS, 1e-4, 0, 0)
    args = (p, g, m, v, 1, S.LR, b1, b2, S.EPS, 1e-4, 0, 0, live)
    assert S.worst_ratio(got, S.adam_ref64(*args), S.adam_bound(*args)) > 1


def _naive_flat_sum(slabs):
    n, P = slabs.shape
    per = -(-n // 4)
    out = np.empty(P, dtype=np.float32)
    for i in range(P):
        q = [np.float32(0)] * 4
        for w in range(4):
            for b in range(w * per, min((w + 1) * per, n)):
                q[w] = np.float32(q[w] + slabs[b, i])
        out[i] = np.float32(np.float32(np.float32(q[0] + q[1]) + q[2]) + q[3])
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 32, 37, 45])
def test_flat_sum_ref32(n):
    """against a scalar loop; inside the textbook bound of the float64 sum; and it tells per = n / 4 from ceil(n / 4)"""
    P = 23
    slabs = rnd(n * P, 40 + n, 1.0).reshape(n, P)
    got = S.flat_sum_ref32(slabs)
    assert got.dtype == np.float32 and got.tobytes() == _naive_flat_sum(slabs).tobytes()
    s64, bound = S.flat_sum_ref64(slabs)
    assert np.all(np.abs(got.astype(np.float64) - s64) <= bound)
    if n == 1:
        assert got.tobytes() == slabs[0].tobytes() and np.all(bound == 0)
    if n % 4:  # the floor split drops the last n % 4 slabs (all of them below 4)
        assert S.flat_sum_ref32(slabs, per=n // 4).tobytes() != got.tobytes()
    if n == 45:  # order matters at all: the reversed slabs give other bits somewhere
        assert S.flat_sum_ref32(slabs[::-1]).tobytes() != got.tobytes()


def test_dead_ranges_of_the_multiscale_plans():
    """the two plans of the dead-layer test: 3 and 6 merged ranges (no plan inr_plan_create accepts has more than 8:
    depth <= 10 gives at most the runs (last stages + head 0), heads 2, 4, 6, (heads 8..), (filters 8..))"""
    from inr_mi355x import _lib as L
    from inr_mi355x import mfn
    from inr_mi355x.engine import MFNEngine
    for depth, want in ((2, 3), (8, 6)):
        eng, tensors, live = S.multiscale(depth)
        assert eng.n_params == max(o + n for o, n in tensors) == live.size
        assert len(S.dead_ranges(tensors, live)) == want
    most = 0
    for depth in range(1, 16):
        try:
            MFNEngine(L.KIND_MSFOURIER, 2 * S.MS_ENC, S.MS_WIDTH, depth, 2, S.MS_ENC)
        except RuntimeError:
            continue
        m = mfn.MultiscaleKFourier(dict(network_input_size=2 * S.MS_ENC, network_output_size=2, network_depth=depth,
                                        network_width=S.MS_WIDTH))
        live = np.zeros(sum(n for _, n, _, _ in m._layout), dtype=bool)
        for (o, n, _, _), lv in zip(m._layout, m._live):
            live[o:o + n] = lv
        most = max(most, len(S.dead_ranges([(o, n) for o, n, _, _ in m._layout], live)))
    assert most == 6
