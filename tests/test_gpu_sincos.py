"""The fused kernels' sines and cosines against float64, element by element -- ``-m gpu``.  Every case of
tests/sincos_cases.py is a network whose public forward returns sin or cos of one exactly known fp32 argument
(tests/test_sincos_host.py has shown that, and that each case lands on the build it names); here the shipped kernels run it
and every output element is compared with float64 sin / cos of that argument.

Bounds -- none fitted to what the device gives:
* sincos_cw call sites (act_fwd<ACT_SIN>, act_gabor / wire_epilogue, act_gabor2d / wire2d_epilogue, mfn_epilogue),
  |t| <= 300 rad: 3.8e-7, the figure in csrc/inr_device.h.
* the same sites, 300 < |t| <= 8192 rad: the same 3.8e-7.  The reduction's error does not grow with |t|:
  k = rint(t c_hi) is an integer, t c_hi - k is exact inside the FMA and rounded once at magnitude <= 1/2 revolution
  (2^-25 rev = 1.9e-7 rad), t c_lo is added in the same FMA, and c_hi + c_lo equals 1 / (2 pi) to 1e-16 relative, i.e.
  8192 / (2 pi) * 1e-16 revolutions at the far end.  What remains is v_sin_f32 / v_cos_f32 on [-1/2, 1/2].
* the one-transcendental layer-0 feature form (gauss_feature, inr_mlp_impl.h): 3.8e-7 + 2 pi 2^-25 = 5.7e-7 -- it reduces
  in radians and multiplies by fl(1 / 2 pi) afterwards (+ 1/4 turn for the cosine half): one more fp32 rounding of an
  argument below one revolution.  Its phases reach 2^7 * 2 pi = 804 rad.
Per case the largest and the mean error are recorded (conftest.record_parity, "sincos:<case id>";
profiles/sincos_parity.jsonl is a condensed copy of the first device run).  Two forwards of a case are equal to the bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sincos_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _forward(p, dev):
    """[calls, rows, 4] through the case's plan: one bind, then the parameters of each call packed in place"""
    eng = p.engine
    eng.bind(p.flats[0].clone().to(dev))
    x = p.x.to(dev).contiguous()
    encB = None if p.encB is None else p.encB.to(dev).contiguous()
    outs = []
    for c, flat in enumerate(p.flats):
        if c:
            eng.params.copy_(flat.to(dev))
            eng.pack()
        if p.dist is not None:
            out = eng.forward(x, encB, dist=p.dist.to(dev))[0]
        else:
            out = eng.forward(x, encB)
        outs.append(out.cpu().clone())
    return torch.stack(outs)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_sincos_against_float64(dev, case, monkeypatch):
    from conftest import record_parity
    monkeypatch.delenv("INR_RS", raising=False)
    p = SC.prepare(case)
    out = _forward(p, dev)
    assert out.shape == (len(p.flats), p.B, 4) and torch.isfinite(out).all()
    ref = np.stack([SC.expected(p, c) for c in range(len(p.flats))])
    t = np.abs(np.stack(p.arg).astype(np.float64))
    err = np.abs(out.numpy().astype(np.float64) - ref)
    far = t > SC.LO_MAX
    e_lo = float(err[~far].max()) if (~far).any() else 0.0
    e_hi = float(err[far].max()) if far.any() else 0.0
    i = np.unravel_index(int(err.argmax()), err.shape)
    print("sincos:" + case.id, "max", float(err.max()), "mean", float(err.mean()), "max |t| <= 300", e_lo, "max |t| > 300",
          e_hi, "bound", case.bound, "worst at t =", float(np.stack(p.arg)[i]), "cos" if p.cos[i[0]][i[2]] else "sin")
    record_parity("sincos:" + case.id, max_err=float(err.max()), mean_err=float(err.mean()), max_err_le300=e_lo,
                  max_err_gt300=e_hi, bound=case.bound, t_max=float(t.max()))
    again = _forward(p, dev)
    assert float(err.max()) <= case.bound, (float(err.max()), case.bound)
    assert torch.equal(again, out)
