"""Deep complex-Gabor cases on the host (no GPU): every case of tests/deep_gabor_cases.py lands on the two-waves-per-group
build it is meant for, with the batch size its name promises; the float64 oracle is a fair judge there (the cap the
conformance matrix applies to its plain cases); and the criterion bites -- fed the fp32 oracle's own results it accepts,
fed three small defects of the kind that lives between layers it rejects, while tests/test_gpu_widths.py::_check at
omega_0 30 / scale 15 accepts two of them: the gap these cases close.

Plans are created and sized without a GPU; the oracle runs in fp32 and float64."""
import ctypes as C
import functools

import pytest
import torch

import deep_gabor_cases as DG
import matrix_cases as MC
from test_gpu_widths import _check

CASES = DG.CASES


@functools.lru_cache(maxsize=None)
def _prep(case):
    return DG.prepare(case)


@functools.lru_cache(maxsize=None)
def _refs(case):
    p = _prep(case)
    return MC.reference(p, torch.float32), MC.reference(p, torch.float64)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_lands_on_its_build(case):
    from inr_mi355x import _lib as L
    p = _prep(case)
    eng = p.engine
    info = L.StepInfo()
    L.check(eng.lib.inr_plan_step_info(eng.plan, p.B, C.byref(info)))
    assert info.hidden_blocks == case.nb and case.nb in (12, 16)
    assert eng.tile_rows == 64 and eng.step_save_by_tile and info.row_split == 0
    assert eng.out_features == 2 and tuple(p.x.shape) == (p.B, 3)
    nt, nb = eng.launch_dims(p.B)
    assert nt == -(-p.B // p.TL)
    if case.B == "base":
        assert nt == 3 and p.B % p.TL != 0
    if case.B == "chunk":
        tiles, n_chunks, tpc = DG.gemm_chunks(eng, p.B)
        assert tiles == nt <= nb
        assert tpc >= 2 and nt % tpc != 0 and p.B % p.TL != 0  # two tiles a chunk, a ragged last chunk, a ragged last tile
        assert n_chunks == -(-nt // tpc) and n_chunks >= 2
        for smaller in range(1, p.B):  # the smallest such batch
            t, _, k = DG.gemm_chunks(eng, smaller)
            assert not (k >= 2 and t % k != 0 and smaller % p.TL != 0), smaller
    if case.B == "grid":
        assert nt > nb and p.B % p.TL == 1  # a second round of the persistent grid, with a ragged tail
        assert eng.workspace(p.B)[1] > nb
    if p.mask is not None:
        assert 0 < p.count < p.B
    assert case.nan <= (case.mask == "random")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_oracle_is_a_fair_judge(case):
    """fp32 against float64: 2.5e-6 on output and flat gradient, 5e-6 on every live tensor (HDR: 5e-6 on the flat
    gradient) -- a quarter of what the device is held to, so a failure there is the device's; every live tensor has a
    gradient to compare; the output rms lies in [0.1, 2]: the regime is tame, not dead.  Then the criterion itself on the
    fp32 oracle's results: it accepts them."""
    p = _prep(case)
    r32, r64 = _refs(case)
    cap = DG.ORACLE_CAP
    assert torch.isfinite(r64[0]).all() and torch.isfinite(r64[2]).all()
    e_out, e_grad = DG.rel_l2(r32[0], r64[0]), DG.rel_l2(r32[2], r64[2])
    worst = max(DG.rel_l2(a, b) for a, b in zip(r32[3], r64[3]))
    rms = float(r64[0].square().mean().sqrt())
    print(case.id, "B", p.B, "out", e_out, "grad", e_grad, "worst tensor", worst, "rms", rms)
    assert e_out <= cap["out"], e_out
    assert e_grad <= (cap["grad_hdr"] if case.loss == "HDR" else cap["grad"]), e_grad
    if case.loss != "HDR":
        assert worst <= cap["tensor"], worst
    assert len(r64[3]) == len(p.model._layout) and all(float(g.norm()) > 0 for g in r64[3])
    assert 0.1 <= rms <= 2.0, rms
    if case.loss == "HDR":  # away from HDR's pole
        assert float((r64[0][0] - p.gt.double()).abs().min()) > 1e-3
    assert DG.verdict(case, r64, r32[0], r32[1], r32[2]) == []


# ---------------------------------------------------------------------------------------------------------------------
# the criterion bites
# ---------------------------------------------------------------------------------------------------------------------
def _trace(p, dtype=torch.float64):
    """the oracle's forward (oracle/inr_oracle.py::wire_forward, wire2d_forward) with its intermediates kept:
    h[k] [B, hid] = output of complex Gabor layer k, dz[k] = d(loss)/d(lin_k) of the unmasked L2 loss, and the weight
    gradients autograd forms from them -- checked against MC.reference by the caller"""
    assert p.case.loss == "L2" and p.mask is None
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    sd = {k: (v.to(cd) if v.is_complex() else v.to(dtype)) for k, v in p.sd.items()}
    depth, two_d = p.case.depth, p.case.family == "WIRE2D"
    h, hs, lins = p.x.to(dtype), [], []
    for k in range(depth + 1):
        lin = h @ sd[f"net.{k}.linear.weight"].t() + sd[f"net.{k}.linear.bias"]
        if k == 0:
            lin.requires_grad_(True)  # (no parameter asks for a gradient here: the first pre-activation is the leaf)
        om, s0 = sd[f"net.{k}.omega_0"], sd[f"net.{k}.scale_0"]
        if two_d:
            orth = h @ sd[f"net.{k}.scale_orth.weight"].t() + sd[f"net.{k}.scale_orth.bias"]
            h = torch.exp(1j * om * lin) * torch.exp(-s0 * s0 * (lin.abs().square() + orth.abs().square()))
        else:
            h = torch.exp(1j * (om * lin) - (s0 * lin).abs().square())
        lins.append(lin)
        hs.append(h)
    out = h @ sd[f"net.{depth + 1}.weight"].t() + sd[f"net.{depth + 1}.bias"]
    if p.net.get("last_tanh", False):
        out = torch.tanh(out)
    loss = MC.pointwise("L2", out.real.contiguous(), p.gt.to(dtype), p.x.to(dtype))
    dz = torch.autograd.grad(loss, lins)
    return [t.detach() for t in hs], [t.detach() for t in dz], loss.detach()


def _tensor_index(p, key):
    keys = [k for k in p.sd if not k.endswith(("omega_0", "scale_0"))]
    return keys.index(key)


def _with_tensor(r, i, new):
    """the flat gradient of reference r with live tensor i replaced by `new` (complex: viewed as (Re, Im) pairs)"""
    parts = [g.clone() for g in r[3]]
    new = torch.view_as_real(new) if new.is_complex() else new
    assert new.numel() == parts[i].numel()
    parts[i] = new.reshape(-1).to(parts[i].dtype)
    return torch.cat(parts)


def _defects(case):
    """{name: flat fp32 gradient with one defect}: the fp32 oracle's gradient with
    (a) the bias gradient of hidden layer 2 scaled by 1 + 1e-4;
    (b) the last row's contribution -- the whole ragged last tile of the chunk batch -- missing from the weight gradient
        of hidden layer 2;
    (c) the weight gradient of hidden layer 2 formed to one part in 10^4 with the activations of layer 0 in place of
        layer 1's: a stash slot read one layer off"""
    p = _prep(case)
    r32, r64 = _refs(case)
    hs, dz, loss = _trace(p)
    assert abs(float(loss) - float(r64[1])) <= 1e-12 * abs(float(r64[1]))
    iw, ib = _tensor_index(p, "net.2.linear.weight"), _tensor_index(p, "net.2.linear.bias")
    dW = dz[2].t() @ hs[1].conj()  # autograd's convention: the gradient of z = h W^T is dZ^T conj(h)
    assert DG.rel_l2(torch.view_as_real(dW).reshape(-1), r64[3][iw]) <= 1e-12
    assert DG.rel_l2(torch.view_as_real(dz[2].sum(0)).reshape(-1), r64[3][ib]) <= 1e-12
    g32 = [g.double() for g in r32[3]]
    row = torch.outer(dz[2][-1], hs[1][-1].conj())
    swapped = dz[2].t() @ hs[0].conj()
    return {
        "a": _with_tensor(r32, ib, g32[ib] * (1 + 1e-4)),
        "b": _with_tensor(r32, iw, g32[iw] - torch.view_as_real(row).reshape(-1)),
        "c": _with_tensor(r32, iw, g32[iw] + 1e-4 * torch.view_as_real(swapped - dW).reshape(-1)),
    }


@pytest.mark.parametrize("family,last", DG.FAMILIES)
def test_the_criterion_rejects_small_defects_between_layers(family, last):
    case = DG.Case(family, 4, last, B="chunk")
    assert case in CASES
    r32, r64 = _refs(case)
    assert DG.verdict(case, r64, r32[0], r32[1], r32[2]) == []
    for name, grad in _defects(case).items():
        bad = DG.verdict(case, r64, r32[0], r32[1], grad)
        print(case.id, name, "flat", DG.rel_l2(grad, r64[2]), "misses", bad)
        assert bad and all(what.startswith("tensor") or what == "grad" for what, _, _ in bad), (name, bad)
    # (a) is invisible in the flat gradient: only the tensor-by-tensor part of the criterion sees it
    assert DG.rel_l2(_defects(case)["a"], r64[2]) <= DG.LIMITS["grad"]


@pytest.mark.parametrize("family", ["WIRE", "WIRE2D"])
def test_factor_times_oracle_error_accepts_them_at_omega_30(family, monkeypatch):
    """the record of the gap: the same network and batch at omega_0 30 / scale 15 (config 3's regime), judged as
    tests/test_gpu_wire.py and tests/test_gpu_configs.py judge it -- FACTOR x the oracle's own fp32 error on the flat
    gradient -- accepts the scaled bias gradient (a) and the dropped last tile (b)"""
    import conftest
    monkeypatch.setattr(conftest, "record_parity", lambda *a, **k: None)  # nothing here was measured on a device
    case = DG.Case(family, 4, omega=30.0, scale=15.0, B="chunk")
    assert case not in CASES
    r32, r64 = _refs(case)
    e_cpu = DG.rel_l2(r32[2], r64[2])
    print(case.id, "oracle fp32 vs float64: flat gradient", e_cpu)
    assert e_cpu > 10 * DG.LIMITS["grad"]  # nothing caps it there
    defects = _defects(case)
    for name in ("a", "b"):
        print(case.id, name, "flat", DG.rel_l2(defects[name], r64[2]), "allowed", 4.0 * e_cpu)
        _check(r32[0], r32[1], defects[name], r32, r64, case.id + ":" + name, plain=False)
        assert DG.verdict(case, r64, r32[0], r32[1], defects[name])  # (the plain criterion would not)


def test_table_covers_what_it_names():
    cs = CASES
    for fam, last in DG.FAMILIES:
        mine = [c for c in cs if (c.family, c.last) == (fam, last)]
        assert {c.depth for c in mine if c.B == "base" and c.loss == "L2" and c.mask == "none"} == {2, 3, 4}
        assert any(c.B == "chunk" and c.depth == 4 for c in mine)
        d4 = [c for c in mine if c.depth == 4 and c.B == "base"]
        assert any(c.mask == "random" and not c.nan for c in d4) and any(c.nan for c in d4)
        assert any(c.loss == "HDR" for c in d4)
    assert all((c.omega, c.scale) in ((1.0, 0.5), (2.0, 1.0)) for c in cs)
    assert [c for c in cs if c.omega == 2.0] == [DG.Case("WIRE", 4, omega=2.0, scale=1.0)]
    assert {(c.family, c.depth) for c in cs if c.B == "grid"} == {("WIRE", 3), ("WIRE2D", 2)}
