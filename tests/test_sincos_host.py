"""The sine / cosine isolation cases on the host (no GPU): every case of tests/sincos_cases.py lands on the kernel build it
names, its network really is one transcendental of the restated fp32 argument, and its arguments cover the range the
case claims -- before any GPU time is spent on it.  Plans are created and sized without a GPU (tests/test_matrix_host.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import sincos_cases as SC


@functools.lru_cache(maxsize=None)
def _prep(case):
    return SC.prepare(case)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_case_lands_on_its_build(case, monkeypatch):
    """the checks of tests/test_matrix_host.py::test_case_lands_on_its_build for a forward call of the base batch"""
    from inr_mi355x import _lib as L
    p = _prep(case)
    eng = p.engine
    assert eng.tile_rows == case.tile_rows == p.TL
    assert eng.out_features == 4
    info = L.StepInfo()
    for rs in ("0", "1"):
        monkeypatch.setenv("INR_RS", rs)
        L.check(eng.lib.inr_plan_step_info(eng.plan, p.B, C.byref(info)))
        assert info.hidden_blocks == case.nb
    nt, nb = eng.launch_dims(p.B)
    assert nt == 3 == nb and p.B == 2 * p.TL + 37
    assert p.x.shape[0] == p.B and all(f.numel() == eng.n_params for f in p.flats)
    assert len(p.flats) == (2 * case.size // 4 if case.site == "feat" else 1)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_network_isolates_the_transcendental(case):
    """The float64 oracle of the isolation network equals np.sin / np.cos of the argument the ORACLE forms to 1e-15:
    nothing but one transcendental lies between the input and the output.  The restated fp32 argument is then that
    argument behind the kernel's fp32 roundings and nothing else: x-input sites -- exactly its one rounding to fp32
    (fl(w z); the filter networks: no rounding at all); gauss features -- within 2^-23 relative: fl(2 pi) for 2 pi
    (2.8e-8) and the rounding of fl(2 pi) x (2^-24), the factor 2^k and the two zero terms being exact.
    (No float64 evaluation of the network can equal sin of the fp32 argument itself to 1e-15: at 800 rad a relative 2^-24
    of the argument is 5e-5.)"""
    p = _prep(case)
    for c in range(len(p.flats)):
        out, t64 = SC.oracle_forward(p, c), SC.oracle_argument(p, c)
        ref = np.where(p.cos[c][None, :], np.cos(t64), np.sin(t64))
        assert out.shape == ref.shape == (p.B, 4)
        assert float(np.abs(out - ref).max()) <= 1e-15, (c, float(np.abs(out - ref).max()))
        t32 = p.arg[c]
        assert t32.dtype == np.float32 and t32.shape == (p.B, 4)
        if case.site == "feat":
            assert (np.abs(t32.astype(np.float64) - t64) <= 2.0 ** -23 * np.abs(t64)).all()
        else:
            assert np.array_equal(t32, t64.astype(np.float32))
        assert float(np.abs(ref).max()) > 0.99  # (a dead network would pass the comparison with zeros)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_argument_range(case):
    p = _prep(case)
    t = np.concatenate([a.astype(np.float64) for a in p.arg])
    lo, hi = case.interval
    assert lo < float(np.abs(t).max()) <= hi, float(np.abs(t).max())
    assert (t > 0).any() and (t < 0).any()
    if case.rng == "hi":
        assert float(np.abs(t).min()) > lo
    else:
        assert (t == 0).any()  # the zero phase
    if case.site == "feat":  # both ranges of the plain call sites, in one case
        assert (np.abs(t) <= SC.LO_MAX).any() and (np.abs(t) > SC.LO_MAX).any()
        assert {bool(v) for cs in p.cos for v in cs} == {True, False}  # the sine half and the cosine half
        k = np.round(t / (2 * np.pi))
        assert float(np.abs(t - k * 2 * np.pi)[np.abs(k) >= 64].min()) < 1e-4  # next to a multiple of 2 pi, far out
    else:
        # the fixed rows: arguments within two ulps of k 2 pi and of (k + 1/2) 2 pi, both signs (fl(w z) steps by up to
        # two ulps of the argument; the filter networks take x itself: one ulp)
        ulp = np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
        for h in (0.0, 0.5):
            k = np.round(t / (2 * np.pi) - h)
            near = (np.abs(t - (k + h) * 2 * np.pi) <= 2 * ulp) & (np.abs(t) > 1)
            assert (near & (t > 0)).any() and (near & (t < 0)).any(), h


def test_table_covers_every_site_and_build():
    import matrix_cases as MC
    have = {(c.site, c.build, c.rng) for c in SC.CASES}
    assert {b for s, b, r in have if s == "feat"} == {b for b, _, _ in MC.MLP_GAUSS} - {"nb8-rs1"}
    for r in ("lo", "hi"):
        assert {b for s, b, q in have if s == "sin" and q == r} == {"nb1", "nb2", "nb4", "nb8", "nb16", "nb16-512"}
        assert {b for s, b, q in have if s == "wire" and q == r} == {b for b, _ in MC.WIRE}
        assert {b for s, b, q in have if s == "wire2d" and q == r} == {b for b, _ in MC.WIRE2D}
        for fam in ("fourier", "gabor"):
            assert {b for s, b, q in have if s == fam and q == r} == {"nb1", "nb4", "nb8", "nb16"}
    assert SC.BOUND_CW == 3.8e-7 and abs(SC.BOUND_FEAT - 5.67e-7) < 1e-9
