"""The conformance matrix on the device -- ``-m gpu``: every case of tests/matrix_cases.py through the shipped kernels,
against the float64 oracle of the same case (tests/test_matrix_host.py has shown that each case lands on the build it
names and that the oracle is a fair judge there).

One axis at a time around a base case per kernel build: out_features 1..4 (fused step AND the forward(save=True) /
backward pair), output activations, four mask kinds (plus NaN in the unsampled rows of gt), five tile-edge batch sizes
(plus run-to-run bit equality and a split predict), the non-L2 losses.

Criteria -- none of them new:
* SIREN with a linear / tanh output and FFN: 1e-5 relative L2 against float64 on output and flat gradient, 1e-5 relative
  on the loss (tests/test_gpu_widths.py::_check, plain), 2e-5 per parameter tensor (tests/test_gpu_layers.py::_hold);
* WIRE, WIRE2D, the filter networks and the sine output: _check(plain=False) = FACTOR x the oracle's own fp32 distance;
* non-L2 losses: 2e-5 on loss and flat gradient against the fp32 oracle (tests/test_gpu_parity.py::
  test_losses_fused_and_tier1; the HDR cases have a few hundred rows, where tests/test_gpu_rs.py documents 2e-5);
* bf16: tests/test_gpu_bf16.py::test_bf16_step_matches_rounding_oracle, every assertion of it.
The measured (e_gpu, e_cpu) pairs are recorded (conftest.record_parity; profiles/matrix_parity.jsonl is a committed copy of
the first device run, condensed: one line per case, {what: [e_gpu, e_cpu]}, three digits)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import matrix_cases as MC  # noqa: E402
import oracle as O  # noqa: E402  (checker only)
from test_gpu_widths import _check, rel_l2  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def run(dev, monkeypatch):
    """case -> Run: the case's plan bound to a device copy of its parameters, under the INR_RS the case names"""

    def make(case):
        if case.rs is None:
            monkeypatch.delenv("INR_RS", raising=False)
        else:
            monkeypatch.setenv("INR_RS", case.rs)
        return Run(MC.prepare(case), dev)

    return make


class Run:
    def __init__(self, p, dev):
        import inr_mi355x as M
        self.p, self.case, self.eng = p, p.case, p.engine
        self.eng.bind(p.model._flat.detach().clone().to(dev))
        self.x = p.x.to(dev)
        self.encB = None if p.encB is None else p.encB.to(dev).contiguous()
        self.gt = p.gt.to(dev)
        self.mask = None if p.mask is None else p.mask.to(torch.uint8).to(dev)
        self.dist = None if p.dist is None else p.dist.to(dev).contiguous()
        self.mfn = p.case.family in MC.MFN
        self.spec = M.LossSpec.from_config({"loss": p.case.loss, "loss_opts": MC.HDR_OPTS})
        self.cons = MC.plan_cons(p)

    def forward(self, x=None, dist=None, save=False):
        """[heads, rows, out_f]"""
        x = self.x if x is None else x
        if self.mfn:
            return self.eng.forward(x, self.encB, save=save, dist=self.dist if dist is None else dist)
        return self.eng.forward(x, self.encB, save=save)[None]

    def step(self, gt=None):
        """the fused step: (loss, flat gradient of the live tensors) on the host"""
        gt = self.gt if gt is None else gt
        kw = dict(count=self.p.count, mask=self.mask, hdr_A=self.p.hdr_A)
        if self.mfn:
            kw.update(dist=self.dist, cons=self.cons)
        loss = self.eng.train_step(self.x, self.encB, gt, self.spec, **kw)
        return loss.cpu().clone(), self.live(self.eng.grads)

    def backward(self, dout):
        if self.mfn:
            return self.live(self.eng.backward(self.x, self.encB, dout.contiguous(), dist=self.dist))
        return self.live(self.eng.backward(self.x, self.encB, dout[0].contiguous()))

    def live(self, flat):
        flat = flat.cpu()
        lay = self.p.model._layout
        live = getattr(self.p.model, "_live", [True] * len(lay))
        return torch.cat([flat[o:o + n] for (o, n, s, c), lv in zip(lay, live) if lv])


def _judge(r, out, loss, grad, tag=""):
    """the case's criterion (module docstring) on output [heads, B, out_f], loss and the live flat gradient"""
    from conftest import record_parity
    case, p = r.case, r.p
    r32, r64 = MC.reference(p, torch.float32), MC.reference(p, torch.float64)
    tag = "matrix:" + case.id + tag
    out = out.cpu()
    if case.loss != "L2":
        for name, got, a32, a64 in (("out", out, r32[0], r64[0]), ("grad", grad, r32[2], r64[2])):
            record_parity(tag, what=name, e_gpu=rel_l2(got, a64), e_cpu=rel_l2(a32, a64), e_gpu_vs_cpu32=rel_l2(got, a32))
        print(tag, "loss", float(loss), float(r32[1]), "grad vs fp32 oracle", rel_l2(grad, r32[2]))
        assert abs(float(loss) - float(r32[1])) <= 2e-5 * abs(float(r32[1])), (float(loss), float(r32[1]))
        assert rel_l2(grad, r32[2]) <= 2e-5, rel_l2(grad, r32[2])
        return
    print(tag, "out", rel_l2(out, r64[0]), rel_l2(r32[0], r64[0]), "grad", rel_l2(grad, r64[2]), rel_l2(r32[2], r64[2]),
          "loss", float(loss), float(r64[1]))
    _check(out, loss, grad, r32, r64, tag, plain=case.plain)
    if case.plain:  # tensor by tensor (a bias vector is a small part of the flat gradient's norm)
        off = 0
        for i, g64 in enumerate(r64[3]):
            n = g64.numel()
            if float(g64.norm()) > 0:
                e = rel_l2(grad[off:off + n], g64)
                assert e <= 2e-5, (tag, "tensor", i, e)
            off += n
        assert off == grad.numel()


def _judge_bf16(r, out, loss, tag=""):
    """tests/test_gpu_bf16.py::test_bf16_step_matches_rounding_oracle for this case's output size, activation and mask"""
    from test_gpu_bf16 import _check_against_rounding_oracle
    case, p, eng = r.case, r.p, r.eng
    st = eng.grad_scale_state()
    mult = st[2]
    assert mult > 0 and np.log2(st[3]) == np.round(np.log2(st[3]))  # the scale is a power of two
    act = case.last or "id"
    dldy = lambda yy: (yy - p.gt) / (p.count * float(case.out_f))  # noqa: E731
    y, ref, amax = O.bf16.siren_bf16_step(p.sd, p.x, p.encB, p.net, dldy, mult, mask=p.mask, last_act=act)
    _, wide, _ = O.bf16.siren_bf16_step(p.sd, p.x, p.encB, p.net, dldy, mult, mask=p.mask, wide_sums=True, last_act=act)
    e_out = float((out.cpu()[0] - y).abs().max())
    sel = slice(None) if p.mask is None else p.mask
    ref_loss = float(0.5 * ((y - p.gt)[sel] ** 2).mean())
    print("matrix:" + case.id + tag, "amax", amax, "out", e_out, "loss", float(loss), ref_loss)
    assert 2.0 ** 3 <= amax <= 2.0 ** 6, amax  # the calibrated scale put the largest |dZ| where it belongs
    assert e_out < 2e-3, e_out
    assert abs(float(loss) - ref_loss) <= 2e-3 * abs(ref_loss), (float(loss), ref_loss)
    rows = _check_against_rounding_oracle(p.model, eng, ref, wide, case.id + tag)
    from conftest import record_parity
    for name, e_dev, e_self in rows:
        record_parity("matrix:" + case.id + tag, what=name, e_gpu=e_dev, e_cpu=e_self)


def _fused(r, tag=""):
    """forward and fused step of the case against its criterion; returns (loss, gradient) of the step"""
    out = r.forward()
    loss, grad = r.step()
    if r.case.bf16:
        _judge_bf16(r, out, loss, tag)
    else:
        _judge(r, out, loss, grad, tag)
    return loss, grad


@pytest.mark.parametrize("case", MC.by_sweep("out"), ids=lambda c: c.id)
def test_output_sizes(run, case):
    """out_features 1..4 (WIRE2D also behind the complex tanh): the fused step, then the tier-1 pair -- forward(save=True),
    d(loss)/d(out) of the L2 loss formed outside, backward -- against the same oracle"""
    r = run(case)
    _fused(r)
    if case.bf16:
        return  # (the bf16 halves have their own scale state: tests/test_gpu_bf16.py::test_bf16_unfused_halves_match_fused)
    out = r.forward(save=True)
    diff = out - r.gt[None]
    loss = 0.5 * (diff.double() ** 2).mean(dim=(1, 2)).sum()
    grad = r.backward(diff / float(r.p.B * case.out_f))
    _judge(r, out, loss, grad, ":tier1")


@pytest.mark.parametrize("case", MC.by_sweep("act"), ids=lambda c: c.id)
def test_last_activations(run, case):
    """SIREN's tanh and sine outputs on nb1, both nb8 kernels and nb16; tanh, sine and sigmoid on the bf16 plans"""
    _fused(run(case))


@pytest.mark.parametrize("case", MC.by_sweep("mask"), ids=lambda c: c.id)
def test_masks(run, case):
    """random / a whole tile of zeros before a ragged tile of ones / exactly one sampled row: count = sampled rows, the
    oracle indexes out[mask], gt[mask]"""
    _fused(run(case))


@pytest.mark.parametrize("case", MC.by_sweep("nan"), ids=lambda c: c.id)
def test_unsampled_rows_do_not_enter_the_loss(run, case):
    """NaN in the rows of gt that the mask excludes (device copy only): loss and gradient equal to the bit those of the
    same call with finite values there -- a kernel that multiplies by zero instead of skipping the row fails"""
    r = run(case)
    loss, grad = _fused(r)
    gt = r.gt.clone()
    gt[~r.mask.bool()] = float("nan")
    loss_nan, grad_nan = r.step(gt)
    assert torch.isfinite(loss_nan).all() and torch.isfinite(grad_nan).all()
    assert torch.equal(loss_nan, loss) and torch.equal(grad_nan, grad)


@pytest.mark.parametrize("case", MC.by_sweep("edge"), ids=lambda c: c.id)
def test_tile_edges(run, case):
    """B = 1, TL - 1, TL, TL + 1 and one tile and a row beyond a full round of the persistent grid.  At the last: loss and
    gradient run-to-run identical to the bit.  At TL + 1: a forward without stash equal to the bit to the same rows split
    as TL and 1"""
    r = run(case)
    loss, grad = _fused(r)
    if case.B == "grid":
        nt, nb = r.eng.launch_dims(r.p.B)
        assert nt > nb
        loss2, grad2 = r.step()
        assert torch.equal(loss2, loss) and torch.equal(grad2, grad)
    if case.B == "TL+1":
        TL = r.p.TL
        whole = r.forward()
        parts = [r.forward(r.x[a:b].contiguous(), None if r.dist is None else r.dist[a:b].contiguous())
                 for a, b in ((0, TL), (TL, TL + 1))]
        assert torch.equal(torch.cat(parts, dim=1), whole)


@pytest.mark.parametrize("case", MC.by_sweep("loss"), ids=lambda c: c.id)
def test_losses(run, case):
    """L1, tanh, LogSpace, HDR, MSLE and a masked HDR: pointwise on nb1, nb16 and a WIRE2D build; the multi-head form with
    the consistency term (weight 0.1, rows on both sides of every disc) on the wide filter kernel"""
    _fused(run(case))
