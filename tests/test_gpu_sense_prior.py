"""The total-variation prior on the image of a SENSE fit on the MI355X (``-m gpu``): inr_image_tv_grad
against the fp32 numpy text of inr_mi355x/sense_prior.py -- the gradient bit for bit, the value to 1e-6 of the float64 sum
of the text's fp32 terms -- and SenseFitTrainer / Reconstructor under ``sense.prior`` with calibrated and with learned
maps against torch's float64 autograd of the whole composite (network, maps, FFT, loss, plus weight * TV).

Criteria -- none of them new (tests/test_gpu_sense_calib.py): bit equality wherever the same arithmetic sees the same
inputs; 1e-5 relative on the loss and 1e-5 relative L2 on a gradient against float64; the flat parameter vector after
three Adam steps within 5e-5 relative L2.

The prior's weight in the fits is chosen on the host, from float64 quantities of step 0 alone: the power of ten nearest to
|d data loss / dI| / |d TV / dI|, so that the prior's gradient is within a decade of the data term's (asserted)."""
import ctypes as Ct
import math

import numpy as np
import pytest
import torch

import oracle as O  # checker only
import sense_calib_cases as CC
import sense_prior_cases as PC
from aux_bits_cases import _stream, dev as to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_PARAMS = 5e-5
TOL_VALUE = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.abs(got).max(initial=0.0))


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np_bits(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    return g.shape == want.shape and np.array_equal(g.view(np.int32), want.view(np.int32))


def _off8(a: np.ndarray) -> torch.Tensor:
    """the array on the device behind a base pointer that is 8 but not 16-byte aligned"""
    buf = torch.empty(a.size + 2, device="cuda")
    view = buf[2:].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


# ---- the kernel against its fp32 text ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)
def test_kernel_equals_its_text(dev, case):
    """write and accumulate: the gradient bit for bit; the value within 1e-6 of the float64 sum of the text's fp32 terms
    and the same bits on a second call; 8- but not 16-byte aligned views give the aligned call's bits; dimg = NULL gives
    the same value and leaves the image alone"""
    from inr_mi355x import _lib as L
    from inr_mi355x import sense_prior as P
    (H, W), eps = case
    img, d0 = PC.image(H, W, eps), PC.dimg0(H, W)
    want_v, want_g = P.image_tv_numpy(img, H, W, PC.WEIGHT, eps)
    _, want_acc = P.image_tv_numpy(img, H, W, PC.WEIGHT, eps, accumulate=True, dimg=d0)
    want64 = float(P.image_tv_terms(img, H, W, eps).astype(np.float64).sum() * (np.float64(np.float32(PC.WEIGHT)) / (H * W)))
    d_img = to_dev(img)
    assert d_img.data_ptr() % 16 == 0
    dimg = torch.full((H * W, 2), 123.25, device=dev)
    out = torch.full((L.LOSS_WORDS,), 123.25, device=dev)
    v = P.image_tv(d_img, H, W, PC.WEIGHT, eps, dimg=dimg, loss_out=out)
    torch.cuda.synchronize()
    assert v.data_ptr() == out.data_ptr() and _np_bits(dimg, want_g), case
    got = float(v)
    print(case, "value", got, "float64 sum of the text's terms", want64, "text", float(want_v))
    assert abs(got - want64) <= TOL_VALUE * abs(want64), (case, got, want64)
    v1 = v.reshape(1).clone()
    # a second call
    dimg2 = torch.empty_like(dimg)
    assert _bits(P.image_tv(d_img, H, W, PC.WEIGHT, eps, dimg=dimg2).reshape(1), v1) and _bits(dimg2, dimg), (case, "twice")
    # accumulate
    acc = to_dev(d0)
    va = P.image_tv(d_img, H, W, PC.WEIGHT, eps, dimg=acc, accumulate=True)
    assert _np_bits(acc, want_acc) and _bits(va.reshape(1), v1), (case, "accumulate")
    # misaligned views: the image, the gradient, both; write and accumulate
    for a_img, a_out in ((_off8(img), torch.empty_like(dimg)), (d_img, _off8(np.zeros_like(want_g))),
                         (_off8(img), _off8(np.zeros_like(want_g)))):
        vo = P.image_tv(a_img, H, W, PC.WEIGHT, eps, dimg=a_out, loss_out=_off8(np.zeros(L.LOSS_WORDS, np.float32)))
        assert _bits(a_out, dimg) and _bits(vo.reshape(1), v1), (case, "off8")
    acc8 = _off8(d0)
    assert _bits(P.image_tv(_off8(img), H, W, PC.WEIGHT, eps, dimg=acc8, accumulate=True).reshape(1), v1)
    assert _np_bits(acc8, want_acc), (case, "off8 accumulate")
    # the value alone
    for a_img in (d_img, _off8(img)):
        assert _bits(P.image_tv(a_img, H, W, PC.WEIGHT, eps).reshape(1), v1), (case, "value only")
    torch.cuda.synchronize()
    assert _np_bits(d_img, img)
    if eps == 0:
        g = dimg.cpu().numpy()
        assert np.isfinite(g).all() and math.isfinite(got) and not g[PC.zero_grad(H, W).reshape(-1)].any()


def test_bad_arguments_leave_the_outputs_alone(dev):
    """host-side argument checks only: every call returns INR_ERR_INVALID (-1) before any launch"""
    from inr_mi355x import _lib as L
    lib = L.load()
    H, W = 4, 6
    img = to_dev(PC.image(H, W, 1e-3))
    sent = 123.25
    dimg = torch.full((H * W, 2), sent, device=dev)
    out = torch.full((L.LOSS_WORDS,), sent, device=dev)
    big = torch.full((H * W + L.LOSS_WORDS, 2), sent, device=dev)
    p = lambda t: t.data_ptr()
    st = _stream()
    f = Ct.c_float
    ok = [p(img), H, W, f(0.5), f(1e-3), 0, p(out), p(dimg)]

    def swap(i, v):
        return ok[:i] + [v] + ok[i + 1:]

    bad = [swap(0, None), swap(6, None)]                                            # a null img or loss_out
    bad += [swap(i, v) for i in (1, 2) for v in (0, -1, (1 << 30) + 1)]             # H or W < 1, or past 2^30
    bad += [ok[:1] + [1 << 21, 1 << 20] + ok[3:]]                                   # H * W above 2^40
    bad += [swap(4, f(v)) for v in (-1e-3, float("nan"), float("inf"), float("-inf"))]  # eps
    bad += [swap(3, f(v)) for v in (float("nan"), float("inf"), float("-inf"))]     # weight
    bad += [swap(5, v) for v in (2, -1)]                                            # accumulate
    bad += [swap(0, p(img) + 4), swap(7, p(dimg) + 4), swap(6, p(out) + 4)]         # alignment (loss_out: 8 bytes)
    bad += [swap(7, p(img)), swap(7, p(img) + 8), swap(6, p(img)), swap(7, p(out)),  # overlap
            ok[:6] + [p(big) + 8 * (H * W - 1), p(big)]]
    for args in bad:
        assert lib.inr_image_tv_grad(*args, st) == -1, args
        assert "inr_image_tv_grad" in L.last_error()
    # ... and with dimg = NULL the same refusals hold
    for args in (ok[:1] + [0, W] + ok[3:7] + [None], ok[:4] + [f(-1.0)] + ok[5:7] + [None], ok[:5] + [3, p(out), None]):
        assert lib.inr_image_tv_grad(*args, st) == -1, args
    torch.cuda.synchronize()
    assert bool((dimg == sent).all()) and bool((out == sent).all()) and bool((big == sent).all())
    assert _np_bits(img, PC.image(H, W, 1e-3))
    assert lib.inr_image_tv_grad(*ok, st) == 0 and lib.inr_image_tv_grad(*ok[:7], None, st) == 0
    torch.cuda.synchronize()


# ---- the trainer -------------------------------------------------------------------------------------------------------
SHAPE = CC.FIT_SHAPE
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)
SNET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)
CALIBRATED = dict(maps="calibrated", calib=dict(size=list(CC.FIT_BLOCK)))
LEARNED = dict(net=dict(network_width=32, network_depth=3), coils_per_step=2)


def _cfg(sense):
    return dict(model="SIREN", loss="L2", lr=1e-3, max_epoch=10, weight_decay=0.0, beta1=0.9, beta2=0.999,
                undersampling="grid-3*2", encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
                net=dict(NET), sense=dict(sense))


def _trainer(dev, base, seed=3, **sense):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    C_, H, W = SHAPE
    return SenseFitTrainer(_cfg(dict(base, **sense)), make_kspace(C_, H, W)[0], grid_coords(C_, H, W, device=dev), SHAPE,
                           dev, seed=seed)


class Ref64:
    """the whole composite in torch float64 on the host, differentiated by autograd: gauss encoder and SIREN image network
    on the plane's rows with the coil column 0; the sensitivities (the trainer's calibrated maps, widened -- or the FFN
    sensitivity network on the group's rows); K = fft2c(scale * S * I); 0.5 MSE on the sampled rows; plus weight * TV(I)
    written with slicing and torch.sqrt (sense_prior_cases.tv_torch); stock torch.optim.Adam with the trainer's per-epoch
    learning rate"""

    def __init__(self, tr, prior):
        d = lambda sd: {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
        C_, self.H, self.W = SHAPE
        self.prior = prior
        self.i, self.Bi = d(tr.model.state_dict()), tr.encoder.B.cpu().double()
        self.s = self.maps = None
        if tr.calib is None:
            self.s, self.Bs = d(tr.sens_model.state_dict()), tr.sens_encoder.B.cpu().double()
        else:
            self.maps = torch.view_as_complex(tr._maps.cpu().double().reshape(C_, self.H, self.W, 2))
        self.cfg = tr.config
        self.opt = torch.optim.Adam(list(self.i.values()) + list((self.s or {}).values()), lr=self.cfg["lr"],
                                    betas=(self.cfg["beta1"], self.cfg["beta2"]), weight_decay=self.cfg["weight_decay"])
        self.coords, self.gt = tr.coords.cpu().double(), tr.image.cpu().double()
        self.img_coords = self.coords[:tr.plane].clone()
        self.img_coords[:, 0] = 0
        self.mask = tr.mask_cpu.reshape(-1).bool()
        self.scale, self.plane, self.groups = tr.sense_scale, tr.plane, tr.groups

    def terms(self, it):
        """(I complex [H,W], data loss, TV of weight 1) of group ``it`` from the current parameters"""
        c0, c1 = self.groups[it]
        lo, hi = c0 * self.plane, c1 * self.plane
        I = torch.view_as_complex(O.siren_forward(self.i, O.encode(self.img_coords, self.Bi, "gauss"), NET)
                                  .reshape(self.H, self.W, 2))
        if self.maps is not None:
            S = self.maps[c0:c1]
        else:
            S = torch.view_as_complex(O.ffn_forward(self.s, O.encode(self.coords[lo:hi], self.Bs, "gauss"), SNET)
                                      .reshape(-1, self.H, self.W, 2))
        K = O.fft2c(torch.view_as_real(self.scale * S * I[None])).reshape(-1, 2)
        sel = self.mask[lo:hi]
        eps = self.prior["eps"] if self.prior else PC.FIT_EPS
        return I, O.loss_l2_half(K[sel], self.gt[lo:hi][sel]), PC.tv_torch(I, 1.0, eps)

    def image_gradient_norms(self, it):
        """(|d data loss / dI|, |d TV / dI|) in float64 at the current parameters: what the weight is chosen from"""
        I, data, tv = self.terms(it)
        gd, = torch.autograd.grad(data, I, retain_graph=True)
        gt, = torch.autograd.grad(tv, I)
        return float(gd.abs().pow(2).sum().sqrt()), float(gt.abs().pow(2).sum().sqrt())

    def step(self, epoch, it):
        for g in self.opt.param_groups:
            g["lr"] = self.cfg["lr"] * 0.2 ** min(epoch / self.cfg["max_epoch"], 1)
        _, data, tv = self.terms(it)
        loss = data + self.prior["weight"] * tv if self.prior else data
        self.opt.zero_grad()
        loss.backward()
        flat = lambda sd: None if sd is None else torch.cat([p.grad.reshape(-1) for p in sd.values()]).numpy().copy()
        out = float(loss.detach()), flat(self.i), flat(self.s)
        self.opt.step()
        return out

    def params(self):
        return torch.cat([v.detach().reshape(-1) for v in self.i.values()]).numpy()


def _decade_weight(tr, it=0):
    """the power of ten nearest to |d data / dI| / |d TV / dI| at the trainer's (untouched) parameters, with both norms"""
    gd, gt = Ref64(tr, None).image_gradient_norms(it)
    assert gd > 0 and gt > 0
    return 10.0 ** round(math.log10(gd / gt)), gd, gt


@pytest.fixture(scope="module")
def fit(dev):
    """calibrated maps: (trainer with the prior after 3 steps, its float64 reference after the same steps, what each step
    gave, the prior-free trainer after 3 steps, the trainer under prior: none after 3 steps)"""
    plain, none = _trainer(dev, CALIBRATED), _trainer(dev, CALIBRATED, prior="none")
    assert plain.prior is None and none.prior is None and not hasattr(plain, "_prior_out")
    weight, gd, gt = _decade_weight(plain)
    ratio = weight * gt / gd
    print(f"calibrated: |d data/dI| {gd:.4e}, |d TV/dI| {gt:.4e}, weight {weight:g}, prior / data gradient {ratio:.3f}")
    assert 0.1 <= ratio <= 10.0  # the prior cannot pass by being negligible, nor by drowning the data term
    tr = _trainer(dev, CALIBRATED, prior=dict(kind="tv", weight=weight, eps=PC.FIT_EPS))
    assert tr.prior == {"kind": "tv", "weight": weight, "eps": PC.FIT_EPS} and tr.groups == [(0, 3)]
    assert _bits(tr.engine.params, plain.engine.params)
    ref = Ref64(tr, tr.prior)
    seen = []
    for epoch in range(3):
        loss = float(tr.step(epoch, 0))
        seen.append((loss, tr.engine.grads.cpu().numpy().copy(), ref.step(epoch, 0)))
        plain.step(epoch, 0)
        none.step(epoch, 0)
    return tr, ref, seen, plain, none


def test_calibrated_steps_against_float64_autograd(fit):
    """loss and the flat gradient of the image network, steps 1 and 2: 1e-5 relative"""
    for n, (loss, g, (l64, g64, _)) in enumerate(fit[2][:2]):
        errs = dict(loss=abs(loss - l64) / abs(l64), image=rel_l2(g, g64))
        print(f"calibrated step {n + 1}: kernels vs float64 autograd {errs}")
        assert np.linalg.norm(g64) > 0
        for k, v in errs.items():
            assert v <= TOL, (n, k, v)


def test_calibrated_three_steps_against_float64_adam(fit):
    tr, ref = fit[:2]
    assert tr.engine.step == 3 and tr.global_step == 3
    got, want = tr.engine.params.cpu().numpy(), ref.params()
    e = rel_l2(got, want)
    print(f"params after 3 steps with the prior: rel L2 {e:.3e}, largest entry difference {np.abs(got - want).max():.3e}")
    assert got.shape == want.shape and e < TOL_PARAMS, e


def test_key_absent_is_todays_fit_and_key_present_is_not(fit):
    tr, _, _, plain, none = fit
    assert _bits(plain.engine.params, none.engine.params) and _bits(plain.engine.exp_avg, none.engine.exp_avg)
    assert _bits(plain.engine.exp_avg_sq, none.engine.exp_avg_sq)
    assert not _bits(tr.engine.params, plain.engine.params)
    assert "prior" not in plain.checkpoint()["sense"] and "prior" not in plain.validate(0) and "prior" not in plain.metrics()


def test_records_carry_the_prior(fit):
    from inr_mi355x import sense_prior as P
    tr, _, _, plain, _ = fit
    C_, H, W = SHAPE
    rec = tr.validate(0)
    img = tr._sweep(tr.engine, tr.enc_B, tr._img_coords, tr.predict_chunk, tr.encoder).cpu().numpy()
    want = float(P.image_tv_numpy(img, H, W, tr.prior["weight"], tr.prior["eps"])[0])
    assert set(rec["prior"]) == {"kind", "weight", "eps", "value"} and want > 0
    assert {k: rec["prior"][k] for k in ("kind", "weight", "eps")} == tr.prior
    assert abs(rec["prior"]["value"] - want) <= TOL_VALUE * want, (rec["prior"], want)
    assert tr.metrics()["prior"] == rec["prior"]
    assert rec["sense"] == plain.validate(0)["sense"] and "prior" not in rec["sense"]
    # the test loss stays data-only: the same number as that of a prior-free trainer holding the same parameters
    plain2 = _trainer(torch.device("cuda:0"), CALIBRATED)
    plain2.load_checkpoint(tr.checkpoint())
    assert rec["test_loss"] == plain2.validate(0)["test_loss"]


def test_checkpoint_round_trip(dev, fit, tmp_path):
    from inr_mi355x.reconstruct import Reconstructor
    tr = fit[0]
    ckpt = tr.checkpoint()
    assert set(ckpt["sense"]) == {"scale", "coils_per_step", "maps", "calib", "block", "prior"}
    assert ckpt["sense"]["prior"] == tr.prior and ckpt["sense"]["prior"] is not tr.prior
    path = str(tmp_path / "model.pt")
    torch.save(ckpt, path)
    rec = Reconstructor(tr.config, path, shape=SHAPE, device=dev)
    want = tr.predict_all()
    images = rec.render()
    assert images.shape == (*SHAPE, 2)
    got = rec.kspace(images)
    assert _bits(got.reshape(-1, 2), want), float((got.reshape(-1, 2) - want).abs().max())
    # resume: under the same prior, under another weight (a record only, as lr is), and without the key
    for sense in (dict(prior=dict(tr.prior)), dict(prior=dict(tr.prior, weight=10 * tr.prior["weight"])), {}):
        b = _trainer(dev, CALIBRATED, **sense)
        b.load_checkpoint(torch.load(path, weights_only=False))
        assert b.engine.step == 3 and _bits(b.engine.params, tr.engine.params) and _bits(b.predict_all(), want)


@pytest.mark.parametrize("it", [0, 1], ids=["group_0_2", "group_2_3"])
def test_learned_maps_step_against_float64_autograd(dev, it):
    """two coil groups; one step of group ``it`` from the initial parameters: loss and both networks' gradients against
    float64 autograd at 1e-5, and the sensitivity network's gradient bit-equal to that of a prior-free step"""
    plain = _trainer(dev, LEARNED)
    assert plain.groups == [(0, 2), (2, 3)] and plain.prior is None
    weight, gd, gt = _decade_weight(plain, it)
    ratio = weight * gt / gd
    print(f"learned, group {it}: |d data/dI| {gd:.4e}, |d TV/dI| {gt:.4e}, weight {weight:g}, prior / data {ratio:.3f}")
    assert 0.1 <= ratio <= 10.0
    tr = _trainer(dev, LEARNED, prior=dict(weight=weight, eps=PC.FIT_EPS))
    assert _bits(tr.engine.params, plain.engine.params) and _bits(tr.sens_engine.params, plain.sens_engine.params)
    ref, ref_plain = Ref64(tr, tr.prior), Ref64(plain, None)
    loss, loss_plain = float(tr.step(0, it)), float(plain.step(0, it))
    l64, gi64, gs64 = ref.step(0, it)
    lp64, gip64, _ = ref_plain.step(0, it)
    gi, gs = tr.engine.grads.cpu().numpy(), tr.sens_engine.grads.cpu().numpy()
    errs = dict(loss=abs(loss - l64) / abs(l64), image=rel_l2(gi, gi64), sens=rel_l2(gs, gs64))
    print(f"learned, group {it}: kernels vs float64 autograd {errs}; the prior moves the image gradient by "
          f"{rel_l2(gi64, gip64):.3f} and the loss by {abs(l64 - lp64) / lp64:.3e}")
    for k, v in errs.items():
        assert v <= TOL, (it, k, v)
    assert loss > loss_plain  # weight * TV > 0 is in the returned loss
    assert _bits(tr.sens_engine.grads, plain.sens_engine.grads)  # the prior does not reach the sensitivity network
    assert not _bits(tr.engine.grads, plain.engine.grads)
    rec = tr.validate(0)
    assert rec["prior"]["weight"] == weight and rec["prior"]["value"] > 0 and "prior" not in rec["sense"]
    assert tr.checkpoint()["sense"]["prior"] == tr.prior and "prior" not in plain.checkpoint()["sense"]
