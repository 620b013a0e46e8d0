"""The conformance matrix on the host (no GPU): every case of tests/matrix_cases.py really lands on the kernel build it
names, and the float64 oracle is a fair judge there -- before any GPU time is spent on it.

Plans are created and sized without a GPU (as tests/test_host.py does); the oracle runs in fp32 and float64."""
import ctypes as C
import functools

import pytest
import torch

import matrix_cases as MC
from test_gpu_widths import _ref, rel_l2


@functools.lru_cache(maxsize=None)
def _prep(case):
    return MC.prepare(case)


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c.id)
def test_case_lands_on_its_build(case, monkeypatch):
    from inr_mi355x import _lib as L
    p = _prep(case)
    eng = p.engine
    assert eng.tile_rows == case.tile_rows
    assert eng.step_save_by_tile == case.gemm
    assert eng.out_features == case.out_f
    info = L.StepInfo()
    for rs in ("0", "1"):
        monkeypatch.setenv("INR_RS", rs)
        L.check(eng.lib.inr_plan_step_info(eng.plan, p.B, C.byref(info)))
        assert info.hidden_blocks == case.nb
        assert info.row_split == (1 if case.rs is not None and rs == "1" else 0)  # only the nb8 gauss plans own the row-split kernel
    nt, nb = eng.launch_dims(p.B)
    assert nt == -(-p.B // p.TL)
    if case.B == "grid":
        assert nt > nb and p.B % p.TL == 1  # a second round of the persistent grid, with a ragged tail
    if case.B == "base":
        assert nt == 3 and p.B % p.TL != 0
    # masks: at least one sampled row; the "tile" kind really blanks a whole tile of THIS plan and samples all of the ragged tail
    if p.mask is not None:
        assert p.count >= 1 and p.mask.shape == (p.B,)
        if case.mask == "random":
            assert 0 < p.count < p.B
        if case.mask == "tile":
            assert not bool(p.mask[p.TL:2 * p.TL].any()) and bool(p.mask[2 * p.TL:].all()) and 0 < p.B - 2 * p.TL < p.TL
        if case.mask == "one":
            assert p.count == 1 and int(p.mask.nonzero()[0]) >= (nt - 1) * p.TL
    if case.family == "BoundedFourier" and case.B in ("base", "grid"):  # rows below, between and above the bounds of every BoundedLinear
        assert int((p.dist < MC.BOUNDS[0]).sum()) > 0 and int((p.dist > MC.BOUNDS[1]).sum()) > 0
        assert int(((p.dist >= MC.BOUNDS[0]) & (p.dist <= MC.BOUNDS[1])).sum()) > 0
    if p.cons is not None:  # the multi-head loss: rows on both sides of every consistency disc, among the sampled ones too
        assert len(p.cons) >= 2 and MC.plan_cons(p).weight == 0.1
        sel = torch.ones(p.B, dtype=torch.bool) if p.mask is None else p.mask
        for lo, hi in p.cons:
            outside = (p.dist < lo) | (p.dist > hi)
            assert int(outside.sum()) > 0 and int((~outside).sum()) > 0
            assert int((outside & sel).sum()) > 0 and int((~outside & sel).sum()) > 0


# The oracle's own fp32-to-float64 distance over the non-plain L2 cases of the table, per family: the largest measured on
# the CPU (16 threads), as (output, flat gradient, loss).  _check(plain=False) accepts FACTOR x this distance, so it is part
# of the criterion: an edit of the table (another omega_0, a deeper or wider case) must not widen it unseen.
#   WIRE                9.5e-07  1.7e-06  2.6e-06
#   WIRE2D              7.9e-07  7.0e-06  4.4e-06   (the gradient: nb2, width 8, one sampled row; 3.8e-06 without the "one" masks)
#   Fourier             1.6e-06  8.3e-07  3.5e-07
#   Gabor               5.1e-08  2.0e-07  1.4e-07
#   MultiscaleKFourier  6.7e-07  4.8e-07  6.9e-07
#   BoundedFourier      7.0e-07  6.4e-07  1.0e-06
#   SIREN, sine output  1.6e-06  1.4e-06  1.9e-07
E_CPU_MAX = {"WIRE": (9.5e-7, 1.7e-6, 2.6e-6), "WIRE2D": (7.9e-7, 7.0e-6, 4.4e-6), "Fourier": (1.6e-6, 8.3e-7, 3.5e-7),
             "Gabor": (5.1e-8, 2.0e-7, 1.4e-7), "MultiscaleKFourier": (6.7e-7, 4.8e-7, 6.9e-7),
             "BoundedFourier": (7.0e-7, 6.4e-7, 1.0e-6), "SIREN": (1.6e-6, 1.4e-6, 1.9e-7)}


@pytest.mark.parametrize("case", [c for c in MC.CASES if not c.bf16], ids=lambda c: c.id)
def test_oracle_is_a_fair_judge(case):
    """plain cases: the fp32 oracle within 2.5e-6 of float64 on output and gradient -- a quarter of the 1e-5 the device is
    held to, so a failure there is the device's.  Non-plain L2 cases, judged by FACTOR x the oracle's own distance: that
    distance at most twice the family's measured maximum (E_CPU_MAX).  Loss cases: |out - gt| stays away from HDR's pole
    and L1's jump, and log(1 + .) of MSLE has an argument."""
    p = _prep(case)
    r32, r64 = MC.reference(p, torch.float32), MC.reference(p, torch.float64)
    assert torch.isfinite(r64[0]).all() and torch.isfinite(r64[2]).all() and float(r64[2].norm()) > 0
    if case.plain and case.loss == "L2":
        assert rel_l2(r32[0], r64[0]) <= 2.5e-6, rel_l2(r32[0], r64[0])
        assert rel_l2(r32[2], r64[2]) <= 2.5e-6, rel_l2(r32[2], r64[2])
    if not case.plain and case.loss == "L2":
        cap = E_CPU_MAX[case.family]
        l32, l64 = float(r32[1]), float(r64[1])
        for name, e, c in (("out", rel_l2(r32[0], r64[0]), cap[0]), ("grad", rel_l2(r32[2], r64[2]), cap[1]),
                           ("loss", abs(l32 - l64) / abs(l64), cap[2])):
            assert e <= 2 * c, (name, e, c)
    if case.loss != "L2":
        sel = slice(None) if p.mask is None else p.mask
        assert float((r64[0][:, sel] - p.gt.double()[sel]).abs().min()) > 1e-3
        if case.loss == "MSLE":
            assert float(r64[0].min()) > -0.95 and float(p.gt.min()) > -0.95
    # every live tensor has a gradient to compare
    assert len(r64[3]) == sum(getattr(p.model, "_live", [True] * len(p.model._layout)))


@pytest.mark.parametrize("family", ["SIREN", "FFN", "WIRE", "WIRE2D", "Fourier", "Gabor"])
def test_matrix_oracle_is_the_suite_s_oracle(family):
    """the matrix's oracle (masks, losses, dist) is tests/test_gpu_widths.py::_ref, to the bit, where _ref applies
    (no mask, L2, no dist)"""
    case = next(c for c in MC.CASES if c.family == family and c.sweep == "out" and c.out_f == 3)
    p = _prep(case)
    for dtype in (torch.float32, torch.float64):
        a = MC.reference(p, dtype)
        b = _ref(family, p.sd, p.net, p.x, p.encB, p.gt, dtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_table_covers_every_axis():
    """each listed build, activation, output size, mask kind and edge B is selected by at least one case"""
    cs = MC.CASES
    have = {(c.family, c.input, c.build) for c in cs}
    for fam in ("SIREN", "FFN"):
        assert {b for f, i, b in have if f == fam and i == "gauss" and not b.startswith("bf16")} == {"nb1", "nb2", "nb4", "nb8-rs0", "nb8-rs1", "nb16",
                                                                        "nb16-512"}
        assert {b for f, i, b in have if f == fam and i == "x"} == {"nb1", "nb8", "nb16"}
    assert {b for f, i, b in have if f == "WIRE"} == {"nb2", "nb4", "nb8", "nb12"}
    assert {b for f, i, b in have if f == "WIRE2D"} == {"nb2", "nb4", "nb8", "nb16"}
    for fam in MC.MFN:
        assert {b for f, i, b in have if f == fam} == {"nb1", "nb16"}
    assert {c.width for c in cs if c.bf16} == {160, 256}
    for key in have:
        mine = [c for c in cs if (c.family, c.input, c.build) == key]
        assert {c.out_f for c in mine if c.sweep == "out"} == {1, 2, 3, 4}, key
        assert {c.mask for c in mine if c.sweep in ("out", "mask")} == {"none", "random", "tile", "one"}, key
        if key[0] != "FFN":  # (FFN's kernels are SIREN's templates with another hidden activation: one tile code)
            assert {c.B for c in mine if c.sweep == "edge"} == {"1", "TL-1", "TL", "TL+1", "grid"}, key
    assert {(c.out_f, c.last) for c in cs if c.family == "WIRE2D" and c.last} == {(1, "ctanh"), (2, "ctanh")}
    for b in ("nb1", "nb8-rs0", "nb8-rs1", "nb16"):
        assert {c.last for c in cs if c.family == "SIREN" and c.input == "gauss" and c.build == b} >= {"", "tanh", "sin"}
    assert {c.last for c in cs if c.bf16} == {"", "tanh", "sin", "sigmoid"}
    assert {"SIREN", "FFN", "WIRE", "WIRE2D", *MC.MFN} == {c.family for c in cs if c.sweep == "nan" and not c.bf16}
    assert any(c.sweep == "nan" and c.bf16 for c in cs)
    for key in (("SIREN", "nb1"), ("SIREN", "nb16"), ("WIRE2D", "nb4"), ("MultiscaleKFourier", "nb16")):
        mine = [c for c in cs if c.sweep == "loss" and (c.family, c.build) == key]
        assert {c.loss for c in mine} == {"L1", "tanh", "LogSpace", "HDR", "MSLE"} and any(c.mask == "random" for c in mine)


# ---- documented refusals: every entry point that evaluates the loss carries them --------------------------------------
def _plan(**kw):
    from inr_mi355x import _lib as L
    plan = C.c_void_p()
    rc = L.load().inr_plan_create(C.byref(L.NetDesc(**kw)), C.byref(plan))
    return rc, plan


def test_ctanh_refused_beyond_two_outputs():
    from inr_mi355x import _lib as L
    kw = dict(kind=L.KIND_WIRE2D, in_features=3, width=8, depth=1, last_act=L.ACT_CTANH, input=L.INPUT_X,
              first_omega_0=10.0, hidden_omega_0=10.0, scale_0=5.0)
    for o in (1, 2):
        rc, plan = _plan(out_features=o, **kw)
        assert rc == 0, L.last_error()
        L.load().inr_plan_destroy(plan)
    for o in (3, 4):
        rc, _ = _plan(out_features=o, **kw)
        assert rc < 0 and "INR_ACT_CTANH" in L.last_error()
    rc, _ = _plan(**dict(kw, kind=L.KIND_WIRE, out_features=2))
    assert rc < 0 and "INR_ACT_CTANH" in L.last_error()


@pytest.mark.parametrize("out_f", [1, 3, 4])
@pytest.mark.parametrize("loss", ["LogSpace", "HDR", "MSLE", "LSL"])
def test_complex_row_losses_need_two_outputs_at_every_entry_point(out_f, loss):
    """inr_train_step, inr_train_adam_step and inr_train_step_multi: INR_ERR_INVALID on the host, before any launch.
    The buffer arguments are made-up addresses that the refusal must precede -- nothing dereferences them on the way to it.
    This test must therefore never carry the gpu mark: on a device a missing refusal would launch on them."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    lib, fake = L.load(), 0x1000
    kind = M.LossSpec.from_config({"loss": loss}).kind
    ld = L.LossDesc(kind=kind, inv_count=1.0 / 64)
    ws = L.Workspace(fake, 1 << 40, fake, 1 << 40)
    rc, plan = _plan(kind=L.KIND_SIREN, in_features=16, width=17, depth=3, out_features=out_f, last_act=L.ACT_ID,
                     input=L.INPUT_GAUSS, enc_size=8, w0=30.0)
    assert rc == 0
    assert lib.inr_train_step(plan, C.byref(ld), fake, fake, fake, fake, fake, None, 64, C.byref(ws), fake, fake, None) == -1
    assert "out_features == 2" in L.last_error()
    assert lib.inr_train_adam_step(plan, C.byref(ld), fake, fake, fake, fake, fake, None, 64, C.byref(ws), fake, fake, fake,
                                   fake, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 1, None) == -1
    assert "out_features == 2" in L.last_error()
    lib.inr_plan_destroy(plan)
    for k in (L.KIND_FOURIER, L.KIND_MSFOURIER):
        rc, plan = _plan(kind=k, in_features=16, width=20, depth=3, out_features=out_f, input=L.INPUT_GAUSS, enc_size=8)
        assert rc == 0
        assert lib.inr_train_step_multi(plan, C.byref(ld), fake, fake, fake, fake, fake, fake, None, 64, C.byref(ws), fake,
                                        fake, None) == -1
        assert "inr_train_step_multi" in L.last_error() and "out_features == 2" in L.last_error()
        lib.inr_plan_destroy(plan)


def test_bf16_plans_take_every_real_output_activation():
    """the bf16 kernels' last-layer epilogue is the fp32 one (act_fwd_rt): linear, sine, tanh and sigmoid outputs are all
    evaluated, and oracle/inr_oracle_bf16.py models each; ReLU is no output activation of any model but the switch covers
    it; anything outside the enum is refused"""
    from inr_mi355x import _lib as L
    kw = dict(kind=L.KIND_SIREN, in_features=64, width=160, depth=3, out_features=2, input=L.INPUT_GAUSS, enc_size=32,
              w0=30.0, precision=L.PRECISION_BF16)
    for act in (L.ACT_ID, L.ACT_SIN, L.ACT_TANH, L.ACT_SIGMOID):
        rc, plan = _plan(last_act=act, **kw)
        assert rc == 0, L.last_error()
        L.load().inr_plan_destroy(plan)
    for act in (5, 6, L.ACT_CTANH, -1):
        rc, _ = _plan(last_act=act, **kw)
        assert rc < 0 and "last_act" in L.last_error()


@pytest.mark.parametrize("act", ["id", "tanh", "sin", "sigmoid"])
def test_bf16_rounding_oracle_output_activations(act):
    """oracle/inr_oracle_bf16.py::last_layer_act: value and derivative of every output activation against autograd in
    float64 (fp32 evaluation: 1e-6 of the values' scale), and the step's default reading of the net's flags"""
    import oracle as O
    z = torch.linspace(-0.2, 0.2, 101)
    y, dy = O.bf16.last_layer_act(z, act)
    zz = z.double().requires_grad_(True)
    ref = {"id": lambda t: t, "tanh": torch.tanh, "sin": lambda t: torch.sin(30.0 * t), "sigmoid": torch.sigmoid}[act](zz)
    (dref,) = torch.autograd.grad(ref.sum(), zz)
    assert float((y.double() - ref.detach()).abs().max()) <= 1e-6
    assert float((dy.double() - dref).abs().max()) <= 1e-6 * max(1.0, float(dref.abs().max()))
    case = next(c for c in MC.CASES if c.bf16 and c.sweep == "act" and c.last == act) if act != "id" else \
        next(c for c in MC.CASES if c.bf16 and c.sweep == "out" and c.out_f == 2)
    p = _prep(case)
    rows_ = slice(0, 64)
    dldy = lambda yy: (yy - p.gt[rows_]) / 128.0  # noqa: E731
    a = O.bf16.siren_bf16_step(p.sd, p.x[rows_], p.encB, p.net, dldy, 2.0 ** 12, last_act=act)
    if act != "sigmoid":  # (no model class says sigmoid: the flags cannot)
        b = O.bf16.siren_bf16_step(p.sd, p.x[rows_], p.encB, p.net, dldy, 2.0 ** 12)
        assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert torch.isfinite(a[0]).all() and all(float(g.norm()) > 0 for g in a[1].values())
