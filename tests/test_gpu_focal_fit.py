"""A focal-frequency-loss fit on the MI355X (``-m gpu``; ``loss: FFL``): INRTrainer's tier-1 step
(forward -> inr_focal_loss_grad -> backward -> Adam) against the same composite in torch float64 with the loss written from
its definition (the weight detached) and stock torch.optim.Adam.

The fit and the criteria are those of tests/test_gpu_gain.py: SIREN 3 x its NET behind a gauss encoder of 16 features,
batches of 200 rows of its SHAPE (the last batch partial), unmasked and under ``radial-4``; step-1 loss and flat gradient
at its 1e-5, parameters after three steps at its relative L2 of 5e-5 -- compared as a norm and not entry by entry for the
reason that file gives (Adam's first steps move an entry by about lr sign(g), so an entry whose gradient is rounding noise
may differ by a good part of a step)."""
import argparse
import json

import numpy as np
import pytest
import torch

import oracle as O  # checker only
from test_gpu_gain import NET, SHAPE, TOL, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


OPTS = dict(ffl_alpha=1.0, ffl_log_matrix=True, ffl_weight=1.0)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="FFL", loss_opts=dict(OPTS), lr=1e-3, batch_size=200, max_epoch=2, weight_decay=0.0,
               beta1=0.9, beta2=0.999, encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(NET))
    cfg.update(kw)
    return cfg


def _trainer(dev, undersampling, **ctor):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    C_, H, W = SHAPE
    image = make_kspace(C_, H, W)[0]
    return INRTrainer(_cfg(undersampling=undersampling), image, grid_coords(C_, H, W, device=dev), SHAPE, dev, seed=3,
                      mask_seed=11, **ctor)


def ffl64(out, gt):
    """the definition in torch float64 on the sampled rows out, gt [N,2]: w detached, no factor 0.5"""
    e = out - gt
    q = (e * e).sum(1)
    n = torch.log(torch.sqrt(q.detach()) + 1.0)
    w = n / n.max() if float(n.max()) > 0 else torch.zeros_like(n)
    return (w.clamp(0.0, 1.0) * q).mean()


class Ref64:
    def __init__(self, tr):
        self.p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in tr.model.state_dict().items()}
        self.B = tr.encoder.B.cpu().double()
        cfg = tr.config
        self.opt = torch.optim.Adam(list(self.p.values()), lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]),
                                    weight_decay=cfg["weight_decay"])
        self.coords, self.gt = tr.coords.cpu().double(), tr.image.cpu().double()
        self.mask = None if tr.mask_cpu is None else tr.mask_cpu.reshape(-1).bool()
        self.bs, self.n = tr.bs, tr.n

    def forward(self, p, coords):
        return O.siren_forward(p, O.encode(coords, self.B, "gauss"), NET)

    def step(self, it):
        lo, hi = it * self.bs, min((it + 1) * self.bs, self.n)
        out = self.forward(self.p, self.coords[lo:hi])
        sel = slice(None) if self.mask is None else self.mask[lo:hi]
        loss = ffl64(out[sel], self.gt[lo:hi][sel])
        self.opt.zero_grad()
        loss.backward()
        flat = torch.cat([p.grad.reshape(-1) for p in self.p.values()]).numpy().copy()
        self.opt.step()
        return float(loss.detach()), flat


@pytest.fixture(scope="module", params=[None, "radial-4"], ids=["full", "radial4"])
def fit(dev, request):
    """(trainer after 3 steps, its float64 twin, what was measured on the way): one fit per mask variant"""
    tr = _trainer(dev, request.param)
    assert tr.steps_per_epoch == 4 and tr._range(3) == (600, 768)  # the last batch is partial
    assert (tr.mask is None) == (request.param is None)
    assert not tr.one_call_steps and not tr.graph_steps and tr.loss.focal is not None
    ref = Ref64(tr)
    seen = {}
    for it in range(3):
        loss = float(tr.step(0, it))
        r_loss, r_g = ref.step(it)
        if it == 0:
            seen["step1"] = (loss, tr.engine.grads.cpu().numpy().copy(), r_loss, r_g)
    return tr, ref, seen


def test_first_step_against_float64_autograd(fit):
    _, _, seen = fit
    loss, g, r_loss, r_g = seen["step1"]
    errs = dict(loss=abs(loss - r_loss) / abs(r_loss), grad=rel_l2(g, r_g))
    print("FFL step 1:", errs, "loss", loss)
    from conftest import record_parity
    record_parity("focal:fit/step1", **errs)
    assert np.linalg.norm(r_g) > 0 and r_loss > 0
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_three_steps_against_float64_adam(fit):
    tr, ref, _ = fit
    assert tr.engine.step == 3 and tr.global_step == 3
    want = torch.cat([v.detach().reshape(-1) for v in ref.p.values()]).numpy()
    got = tr.engine.params.cpu().numpy()
    e = rel_l2(got, want)
    print(f"FFL params after 3 steps: rel L2 {e:.3e}, largest entry difference {np.abs(got - want).max():.3e}")
    from conftest import record_parity
    record_parity("focal:fit/params3", rel_l2=e)
    assert got.shape == want.shape and e < 5e-5, e


def test_validation_loss_and_records(fit):
    """validate(): test_loss = the float64 restatement over the sequential validation batches (full data, no mask) of the
    float64 forward at the trainer's parameters, summed, over the train loader's length; every record carries `focal`"""
    from inr_mi355x.focal import focal_loss_numpy
    tr, ref, _ = fit
    rec = tr.validate(0)
    p = {k: v.detach().cpu().double() for k, v in tr.model.state_dict().items()}
    pred = ref.forward(p, ref.coords).numpy()
    full = tr.image_full.cpu().double().numpy()
    total = 0.0
    for lo in range(0, tr.n, tr.bs):
        hi = min(lo + tr.bs, tr.n)
        total += focal_loss_numpy(tr.loss.focal, pred[lo:hi], full[lo:hi], hi - lo)[0]
    want = total / tr.steps_per_epoch
    print("FFL test_loss", rec["test_loss"], "float64", want)
    assert np.isfinite(rec["test_loss"]) and abs(rec["test_loss"] - want) <= TOL * abs(want)
    assert rec["focal"] == dict(alpha=1.0, log_matrix=True, loss_weight=1.0) == tr.focal_summary
    assert tr.val_history[-1]["focal"] == rec["focal"] and tr.metrics()["focal"] == rec["focal"]


def test_final_json_line_carries_focal(dev, tmp_path, capsys):
    from inr_mi355x.cli import run_cli
    tr = _trainer(dev, None)
    opts = argparse.Namespace(output_path=str(tmp_path), val=False, save_images=False, max_steps=2, band_report=None)
    run_cli(tr, tr.config, opts)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["steps"] == 2 and res["focal"] == dict(alpha=1.0, log_matrix=True, loss_weight=1.0) and np.isfinite(res["psnr"])


def test_resume_is_bit_identical(dev, fit):
    """save after 2 steps, load into a fresh trainer, one more step on each: parameters and Adam moments equal to the bit
    -- and to the uninterrupted fit's; the checkpoint has the plain fit's three entries"""
    tr3, _, _ = fit
    und = tr3.config["undersampling"]
    a = _trainer(dev, und)
    a.fit(2)
    ckpt = a.checkpoint()
    assert sorted(ckpt) == ["enc", "net", "opt"]
    b = _trainer(dev, und)
    b.load_checkpoint(ckpt)
    assert b.engine.step == 2
    a.step(0, 2)
    b.step(0, 2)
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert _bits(getattr(a.engine, name), getattr(b.engine, name)), name
    assert _bits(a.engine.params, tr3.engine.params)


def test_two_ranks_are_refused(dev):
    with pytest.raises(NotImplementedError, match="more than one rank"):
        _trainer(dev, None, rank=0, world=2)
