"""Deep complex-Gabor networks at full width on the device -- ``-m gpu``: every case of tests/deep_gabor_cases.py through the
two-waves-per-group kernels (WIRE nb12, WIRE2D nb16) and the batch dW GEMM, against the float64 oracle of the same case.
tests/test_deep_gabor_host.py has shown that each case lands on its build, that the fp32 oracle stays within 2.5e-6 of
float64 there, and that the criterion rejects a bias gradient off by 1e-4, a dropped last tile and a stash slot read one
layer off.

Criteria, all against float64 (deep_gabor_cases.LIMITS): forward(save=False) output 1e-5 relative L2; fused train_step
loss 1e-5 relative, flat gradient 1e-5, every parameter tensor 2e-5; the forward(save=True) / backward pair the same;
HDR: loss and flat gradient 2e-5.  NaN behind the mask: bit equality with the finite run.  chunk and grid batches:
run-to-run bit equality, additivity over a ragged split at 5e-6 (tests/test_gpu_configs.py), a bit-equal split predict at
TL + 1.  Depth-4 base cases: one adam_step, then a forward at 1e-5 against the oracle on the updated parameters.
The measured (e_gpu, e_cpu) pairs are recorded (conftest.record_parity; profiles/deep_gabor_parity.jsonl is a committed copy,
condensed: one line per case, {what: [e_gpu, e_cpu]}, three digits).

Measured on an MI355X, the largest error against float64 over all cases, fused and tier-1 (the oracle's own fp32 distance
at the same place in brackets); the module takes 5 s:
                 output           flat gradient    worst tensor     HDR flat gradient   additivity
  WIRE 1 / 0.5   1.7e-6 (1.3e-6)  2.5e-7 (2.1e-7)  7.6e-7 (5.9e-7)  3.1e-6 (1.3e-6)     2.0e-7
  WIRE 2 / 1     2.3e-6 (1.8e-6)  1.9e-6 (1.5e-6)  2.3e-6 (1.9e-6)
  WIRE2D         8.2e-7 (5.8e-7)  2.3e-7 (1.4e-7)  6.8e-7 (3.1e-7)  3.7e-6 (3.1e-7)     2.3e-7
  WIRE2D, tanh   1.3e-6 (8.3e-7)  4.2e-7 (2.1e-7)  7.3e-7 (3.5e-7)  7.9e-7 (1.1e-6)     9.8e-8
and 1.6e-7 / 1.3e-7 / 5.9e-8 on the output after the Adam step (1.2e-6 at 2 / 1)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import deep_gabor_cases as DG  # noqa: E402
import matrix_cases as MC  # noqa: E402
from test_gpu_matrix import Run  # noqa: E402

CASES = DG.CASES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _refs(case):
    """(fp32, float64) oracle results of the case: computed once, shared by every test of it, never written to"""
    p = DG.prepare(case)
    return MC.reference(p, torch.float32), MC.reference(p, torch.float64)


def _run(case, dev):
    return Run(DG.prepare(case), dev)  # (a fresh model and plan per test: the Adam test changes its parameters)


def _judge(case, out, loss, grad, tag):
    """record every measurement with the oracle's own fp32 distance beside it, print, then hold the criterion"""
    from conftest import record_parity
    r32, r64 = _refs(case)
    got = DG.measure(case, r64, out.cpu(), loss, grad)
    own = {w: e for w, e, _ in DG.measure(case, r64, r32[0], r32[1], r32[2])}
    for what, e, lim in got:
        record_parity("deep_gabor:" + case.id + tag, family=case.name, what=what, e_gpu=e, e_cpu=own[what], limit=lim)
    print("deep_gabor:" + case.id + tag, " ".join(f"{w} {e:.2e}/{own[w]:.1e}" for w, e, _ in got))
    bad = [m for m in got if not m[1] <= m[2]]
    assert not bad, (case.id + tag, bad)


def _dout(r, out):
    """d(loss)/d(out) of the case's loss, formed outside the fused step: the L2 half-mean by hand (zero on unsampled
    rows), HDR through the tier-1 loss kernel"""
    case, p = r.case, r.p
    if case.loss == "HDR":
        loss, dout = r.eng.loss_grad(r.spec, out[0].contiguous(), r.gt, p.count, mask=r.mask, hdr_A=p.hdr_A)
        return loss.cpu().clone(), dout[None]
    diff = out - r.gt[None]
    if r.mask is not None:
        diff = diff * r.mask.bool()[None, :, None]
    loss = 0.5 * (diff.double() ** 2).sum() / float(p.count * DG.OUT_F)
    return loss.cpu(), diff / float(p.count * DG.OUT_F)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_fused_step_and_tier1_pair(dev, case):
    """forward without stash, the fused step, then forward(save=True) / backward -- each against float64.  NaN cases:
    the step again with NaN in the unsampled rows of gt, equal to the bit.  chunk and grid cases: the step again, equal
    to the bit (chunk partials and the split step's two GEMM launches sum in a fixed order); the two parts of a ragged
    split, with the whole batch's count, add up to it within 5e-6; TL + 1 rows predicted whole and as TL and 1, equal to
    the bit."""
    from conftest import record_parity
    r = _run(case, dev)
    out = r.forward()
    loss, grad = r.step()
    _judge(case, out, loss, grad, "")
    out1 = r.forward(save=True)
    loss1, dout = _dout(r, out1)
    _judge(case, out1, loss1, r.backward(dout), ":tier1")
    if case.nan:
        gt = r.gt.clone()
        gt[~r.mask.bool()] = float("nan")
        loss_nan, grad_nan = r.step(gt)
        assert torch.isfinite(loss_nan).all() and torch.isfinite(grad_nan).all()
        assert torch.equal(loss_nan, loss) and torch.equal(grad_nan, grad)
    if case.B in ("chunk", "grid"):
        eng, B, TL = r.eng, r.p.B, r.p.TL
        loss2, grad2 = r.step()
        assert torch.equal(loss2, loss) and torch.equal(grad2, grad)
        cut = (B * 4 // 9) | 1  # ragged on both sides: neither part is a whole number of tiles
        assert cut % TL != 0 and (B - cut) % TL != 0
        parts = []
        for a, b in ((0, cut), (cut, B)):
            l_ = eng.train_step(r.x[a:b].contiguous(), None, r.gt[a:b].contiguous(), r.spec, count=B)
            parts.append((float(l_), r.live(eng.grads)))
        e_add = DG.rel_l2(parts[0][1] + parts[1][1], grad)
        e_loss = abs(parts[0][0] + parts[1][0] - float(loss)) / abs(float(loss))
        record_parity("deep_gabor:" + case.id, family=case.name, what="additivity", e_gpu=e_add, loss_e_gpu=e_loss)
        print("deep_gabor:" + case.id, "additivity", e_add, e_loss)
        assert e_loss <= 5e-6 and e_add < 5e-6, (e_loss, e_add)
        whole = r.forward(r.x[:TL + 1].contiguous())
        halves = [r.forward(r.x[a:b].contiguous()) for a, b in ((0, TL), (TL, TL + 1))]
        assert torch.equal(torch.cat(halves, dim=1), whole)
        assert torch.equal(whole, out[:, :TL + 1])


@pytest.mark.parametrize("case", [c for c in CASES if c.depth == 4 and c.B == "base" and c.loss == "L2" and c.mask == "none"],
                         ids=lambda c: c.id)
def test_adam_step_repacks_complex_weights(dev, case):
    """one fused step and one adam_step (every parameter moves by about lr = 1e-3: the first step of Adam), then a
    forward from the re-packed weight images against the oracle on the updated parameters: 1e-5"""
    from conftest import record_parity
    r = _run(case, dev)
    p = r.p
    before = r.forward().cpu()
    r.step()
    r.eng.adam_step(1e-3, 0.9, 0.999, 1e-8, 0.0)
    out = r.forward().cpu()
    with torch.no_grad():
        p.model._flat.copy_(r.eng.params.cpu())  # the model's parameters are views of its flat buffer
    moved = (p.model._flat - torch.cat([MC._real(p.sd[k]).reshape(-1) for k in p.sd
                                        if not k.endswith(("omega_0", "scale_0"))])).abs()
    assert 0.9e-3 <= float(moved.median()) <= 1.1e-3
    p.sd = {k: v.detach().clone() for k, v in p.model.state_dict().items()}
    o32, o64 = (torch.stack(MC.forward(p, dt)).detach() for dt in (torch.float32, torch.float64))
    e, e_cpu = DG.rel_l2(out, o64), DG.rel_l2(o32, o64)
    record_parity("deep_gabor:" + case.id + ":adam", family=case.name, what="out", e_gpu=e, e_cpu=e_cpu, limit=1e-5)
    print("deep_gabor:" + case.id + ":adam", e, e_cpu, "moved the output by", DG.rel_l2(before, o64))
    assert DG.rel_l2(before, o64) > 1e-3  # (stale weight images would pass nothing)
    assert e <= 1e-5, e
