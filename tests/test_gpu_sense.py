"""SENSE-model fits on the MI355X (``-m gpu``): inr_sense_apply / inr_sense_grad against the fp32 numpy
text of inr_mi355x/sense.py bit for bit, and SenseFitTrainer / Reconstructor against torch float64 autograd of the
composite loss(fft2c(scale * S * I)).

Criteria -- none of them new: bit equality wherever the same arithmetic sees the same inputs; 1e-5 relative L2 per
array and 1e-5 relative on the loss against float64 (the plain criterion of tests/test_gpu_matrix.py); parameters after
three steps as tests/test_gpu_configs.py::test_config1_siren_image_space compares them (relative L2 of the flat vector
below 5e-5).  The step goes through an fp32 FFT and its inverse, which no other step here does; the plain criteria hold
all the same (DESIGN.md 4.28 has the figures).  Beside every figure the tests print and record what torch's own fp32
chain (the same composite in torch float32 on the host, same weights and inputs) measures against float64 in the same
run: a diagnostic, not part of any bound."""
import ctypes as Ct
import re

import numpy as np
import pytest
import torch

import oracle as O  # checker only
import sense_cases as SC
from aux_bits_cases import _stream, dev as to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_PARAMS = 5e-5


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


# ---- the kernels against their fp32 text -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SC.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_fp32_text_bit_for_bit(dev, shape):
    """both kernels, shift 0 and 1; a second call gives the same bits"""
    from inr_mi355x import sense as S
    G, H, W = shape
    img, sens, gx = SC.inputs(G, H, W)
    di, ds, dg = to_dev(img), to_dev(sens), to_dev(gx)
    for shift in (0, 1):
        x = S.sense_apply(di, ds, G, H, W, SC.SCALE, shift)
        dimg, dsens = S.sense_grad(di, ds, dg, G, H, W, SC.SCALE, shift)
        torch.cuda.synchronize()
        assert _np_bits(x, S.sense_apply_numpy(img, sens, G, H, W, SC.SCALE, shift)), (shape, shift, "x")
        want_i, want_s = S.sense_grad_numpy(img, sens, gx, G, H, W, SC.SCALE, shift)
        assert _np_bits(dimg, want_i), (shape, shift, "dimg")
        assert _np_bits(dsens, want_s), (shape, shift, "dsens")
        x2 = S.sense_apply(di, ds, G, H, W, SC.SCALE, shift)
        dimg2, dsens2 = S.sense_grad(di, ds, dg, G, H, W, SC.SCALE, shift)
        assert _bits(x2, x) and _bits(dimg2, dimg) and _bits(dsens2, dsens), (shape, shift, "twice")


def _off8(a: np.ndarray) -> torch.Tensor:
    """the array on the device behind a base pointer that is 8 but not 16-byte aligned"""
    buf = torch.empty(a.size + 2, device="cuda")
    view = buf[2:].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


@pytest.mark.parametrize("shape", [(4, 8, 12), (3, 129, 260)], ids=lambda s: "x".join(map(str, s)))
def test_alignment_changes_no_bit(dev, shape):
    """shapes of the 16-byte path from base pointers offset by 8 bytes (inputs, then outputs as well): the 8-byte accesses
    give the bits of the 16-byte ones"""
    from inr_mi355x import sense as S
    G, H, W = shape
    img, sens, gx = SC.inputs(G, H, W, seed=3)
    di, ds, dg = to_dev(img), to_dev(sens), to_dev(gx)
    assert all(t.data_ptr() % 16 == 0 for t in (di, ds, dg))
    for shift in (0, 1):
        x = S.sense_apply(di, ds, G, H, W, SC.SCALE, shift)
        dimg, dsens = S.sense_grad(di, ds, dg, G, H, W, SC.SCALE, shift)
        assert all(t.data_ptr() % 16 == 0 for t in (x, dimg, dsens))
        oi, os_, og = _off8(img), _off8(sens), _off8(gx)
        assert _bits(S.sense_apply(oi, os_, G, H, W, SC.SCALE, shift), x)
        a, b = S.sense_grad(oi, os_, og, G, H, W, SC.SCALE, shift)
        assert _bits(a, dimg) and _bits(b, dsens)
        ox, odi, ods = _off8(np.zeros((G, H, W, 2), np.float32)), _off8(np.zeros_like(img)), _off8(np.zeros_like(sens))
        assert _bits(S.sense_apply(di, ds, G, H, W, SC.SCALE, shift, out=ox), x)
        a, b = S.sense_grad(di, ds, dg, G, H, W, SC.SCALE, shift, dimg=odi, dsens=ods)
        assert _bits(a, dimg) and _bits(b, dsens)


def test_bad_arguments_leave_the_outputs_alone(dev):
    """host-side argument checks only: every call returns INR_ERR_INVALID before any launch"""
    from inr_mi355x import _lib as L
    lib = L.load()
    G, H, W = 2, 4, 6
    img, sens, gx = (to_dev(a) for a in SC.inputs(G, H, W))
    sent = 123.25
    x, dimg, dsens = (torch.full(s, sent, device=dev) for s in ((G, H, W, 2), (H * W, 2), (G * H * W, 2)))
    p = lambda t: t.data_ptr()
    st = _stream()
    f = Ct.c_float
    ok_a = [p(img), p(sens), G, H, W, f(0.5), 1, p(x)]
    ok_g = [p(img), p(sens), p(gx), G, H, W, f(0.5), 1, p(dimg), p(dsens)]

    def variants(ok, pointers, g_at):
        out = []
        for i in pointers:
            out.append(ok[:i] + [None] + ok[i + 1:])      # a null pointer
            out.append(ok[:i] + [ok[i] + 4] + ok[i + 1:])  # a pointer that is not 8-byte aligned
        for off, bad in ((0, 0), (0, -1), (1, 0), (1, -3), (2, 0), (2, -2)):  # G, H, W < 1
            out.append(ok[:g_at + off] + [bad] + ok[g_at + off + 1:])
        for bad in (float("inf"), float("-inf"), float("nan")):  # a non-finite scale
            out.append(ok[:g_at + 3] + [f(bad)] + ok[g_at + 4:])
        for bad in (2, -1):  # shift outside {0, 1}
            out.append(ok[:g_at + 4] + [bad] + ok[g_at + 5:])
        return out

    for args in variants(ok_a, (0, 1, 7), 2):
        assert lib.inr_sense_apply(*args, st) == -1, args
        assert "inr_sense_apply" in L.last_error()
    for args in variants(ok_g, (0, 1, 2, 8, 9), 3):
        assert lib.inr_sense_grad(*args, st) == -1, args
        assert "inr_sense_grad" in L.last_error()
    # extents the 64-bit index arithmetic is not sized for: H or W above 2^30, G * H * W above 2^40
    for g_, h_, w_ in ((G, (1 << 30) + 1, 1), (G, 1, (1 << 30) + 1), (4, 1 << 20, 1 << 19)):
        assert lib.inr_sense_apply(p(img), p(sens), g_, h_, w_, f(0.5), 1, p(x), st) == -1 and "2^40" in L.last_error()
        assert lib.inr_sense_grad(p(img), p(sens), p(gx), g_, h_, w_, f(0.5), 1, p(dimg), p(dsens), st) == -1
    # an output that overlaps an input or the other output (a shifted write has no in-place form)
    for args in ((p(img), p(sens), G, H, W, f(0.5), 1, p(sens)), (p(x), p(sens), G, H, W, f(0.5), 0, p(x)),
                 (p(img), p(sens), G, H, W, f(0.5), 1, p(sens) + 8)):
        assert lib.inr_sense_apply(*args, st) == -1 and "overlaps" in L.last_error(), args
    for args in ((p(img), p(sens), p(gx), G, H, W, f(0.5), 1, p(img), p(dsens)),
                 (p(img), p(sens), p(gx), G, H, W, f(0.5), 1, p(dimg), p(sens)),
                 (p(img), p(sens), p(gx), G, H, W, f(0.5), 0, p(dimg), p(gx)),
                 (p(img), p(sens), p(gx), G, H, W, f(0.5), 1, p(dsens) + 8, p(dsens))):
        assert lib.inr_sense_grad(*args, st) == -1 and "overlaps" in L.last_error(), args
    torch.cuda.synchronize()
    for buf in (x, dimg, dsens):
        assert bool((buf == sent).all())
    assert bool((sens == to_dev(SC.inputs(G, H, W)[1])).all()) and bool((gx == to_dev(SC.inputs(G, H, W)[2])).all())


# ---- the composite step ------------------------------------------------------------------------------------------------
SHAPE = (3, 12, 10)
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=64)
SNET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=64)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, max_epoch=10, weight_decay=0.0, beta1=0.9, beta2=0.999,
               undersampling="grid-3*2",
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3), net=dict(NET),
               sense=dict(net=dict(network_width=64, network_depth=3)))
    cfg.update(kw)
    return cfg


def _trainer(dev, shape=SHAPE, seed=3, **sense):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    C_, H, W = shape
    cfg = _cfg()
    cfg["sense"] = dict(cfg["sense"], **sense)
    return SenseFitTrainer(cfg, make_kspace(C_, H, W)[0], grid_coords(C_, H, W, device=dev), shape, dev, seed=seed)


class Ref:
    """the composite in torch on the host, float64 (the reference) or float32 (torch's own fp32 chain): gauss encoders,
    SIREN image network on the plane's rows with the coil column 0, FFN sensitivity network on the group's rows,
    K = fft2c(scale * S * I), 0.5 MSE on the sampled rows, one stock torch.optim.Adam over both networks' parameters with
    the trainer's per-epoch learning rate"""

    def __init__(self, tr, dtype):
        d = lambda sd: {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in sd.items()}
        self.i, self.s = d(tr.model.state_dict()), d(tr.sens_model.state_dict())
        self.Bi, self.Bs = tr.encoder.B.cpu().to(dtype), tr.sens_encoder.B.cpu().to(dtype)
        self.cfg = tr.config
        self.opt = torch.optim.Adam(list(self.i.values()) + list(self.s.values()), lr=self.cfg["lr"],
                                    betas=(self.cfg["beta1"], self.cfg["beta2"]), weight_decay=self.cfg["weight_decay"])
        self.coords, self.gt = tr.coords.cpu().to(dtype), tr.image.cpu().to(dtype)
        self.img_coords = self.coords[:tr.plane].clone()
        self.img_coords[:, 0] = 0
        self.mask = tr.mask_cpu.reshape(-1).bool()
        self.scale, self.plane, self.groups = tr.sense_scale, tr.plane, tr.groups
        self.H, self.W = int(tr.shape[1]), int(tr.shape[2])

    @staticmethod
    def kspace(i, s, Bi, Bs, img_coords, coords, scale, H, W):
        I = torch.view_as_complex(O.siren_forward(i, O.encode(img_coords, Bi, "gauss"), NET).reshape(H, W, 2))
        S = torch.view_as_complex(O.ffn_forward(s, O.encode(coords, Bs, "gauss"), SNET).reshape(-1, H, W, 2))
        return O.fft2c(torch.view_as_real(scale * S * I[None])).reshape(-1, 2)

    def step(self, epoch, it):
        c0, c1 = self.groups[it]
        lo, hi = c0 * self.plane, c1 * self.plane
        for g in self.opt.param_groups:
            g["lr"] = self.cfg["lr"] * 0.2 ** min(epoch / self.cfg["max_epoch"], 1)
        K = self.kspace(self.i, self.s, self.Bi, self.Bs, self.img_coords, self.coords[lo:hi], self.scale, self.H, self.W)
        sel = self.mask[lo:hi]
        loss = O.loss_l2_half(K[sel], self.gt[lo:hi][sel])
        self.opt.zero_grad()
        loss.backward()
        flat = lambda sd: torch.cat([p.grad.reshape(-1) for p in sd.values()]).double().numpy().copy()
        out = float(loss.detach()), flat(self.i), flat(self.s)
        self.opt.step()
        return out

    def params(self):
        flat = lambda sd: torch.cat([v.detach().reshape(-1) for v in sd.values()]).double().numpy()
        return flat(self.i), flat(self.s)


@pytest.fixture(scope="module", params=[3, 2], ids=["G3", "G2_last_group_smaller"])
def fit(dev, request):
    """(trainer after 3 steps, the float64 and float32 host references after the same steps, step 1's figures)"""
    tr = _trainer(dev, coils_per_step=request.param)
    assert tr.mask is not None and tr.groups == ([(0, 3)] if request.param == 3 else [(0, 2), (2, 3)])
    assert 0 < int(tr.mask_cpu.sum()) < tr.n  # grid-3*2: some rows sampled, most not
    r64, r32 = Ref(tr, torch.float64), Ref(tr, torch.float32)
    steps = [(0, 0), (1, 0), (2, 0)] if request.param == 3 else [(0, 0), (0, 1), (1, 0)]
    seen = []
    for epoch, it in steps:
        loss = float(tr.step(epoch, it))
        seen.append((loss, tr.engine.grads.cpu().numpy().copy(), tr.sens_engine.grads.cpu().numpy().copy(),
                     r64.step(epoch, it), r32.step(epoch, it)))
    return tr, r64, r32, seen


def test_steps_against_float64_autograd(fit):
    """loss and the flat gradients of both engines, step 1 (and step 2, the smaller last group when G = 2): 1e-5"""
    _, _, _, seen = fit
    for n, (loss, gi, gs, (l64, gi64, gs64), (l32, gi32, gs32)) in enumerate(seen[:2]):
        errs = dict(loss=abs(loss - l64) / abs(l64), image=rel_l2(gi, gi64), sens=rel_l2(gs, gs64))
        torch32 = dict(loss=abs(l32 - l64) / abs(l64), image=rel_l2(gi32, gi64), sens=rel_l2(gs32, gs64))
        print(f"step {n + 1}: kernels vs float64 {errs}; torch fp32 chain vs float64 {torch32}")
        from conftest import record_parity
        record_parity(f"sense:step{n + 1}", **{"e_" + k: v for k, v in errs.items()},
                      **{"torch32_" + k: v for k, v in torch32.items()})
        assert np.linalg.norm(gi64) > 0 and np.linalg.norm(gs64) > 0
        for k, v in errs.items():
            assert v <= TOL, (n, k, v, torch32[k])


def test_three_steps_against_float64_adam(fit):
    """the parameters of both networks after 3 steps: relative L2 of the flat vector below 5e-5, per engine, against
    stock float64 Adam"""
    tr, r64, r32, _ = fit
    assert tr.engine.step == 3 and tr.sens_engine.step == 3
    for name, eng, want, t32 in zip(("image", "sens"), (tr.engine, tr.sens_engine), r64.params(), r32.params()):
        got = eng.params.cpu().numpy()
        e, e32 = rel_l2(got, want), rel_l2(t32, want)
        print(f"params after 3 steps, {name}: rel L2 {e:.3e} (torch fp32 chain {e32:.3e}), largest entry difference "
              f"{np.abs(got - want).max():.3e}")
        assert got.shape == want.shape and e < TOL_PARAMS, (name, e, e32)


def test_predict_all_is_the_shifted_transform_of_the_product(dev, fit):
    from inr_mi355x.sense import sense_apply
    tr = fit[0]
    C_, H, W = SHAPE
    got = tr.predict_all()
    img = tr.engine.forward(tr._img_in, tr.enc_B, save=False)
    want, sens = [], []
    for c0, c1 in tr.groups:  # the sweep goes group by group: one group's sensitivities and coil images at a time
        sens.append(tr.sens_engine.forward(tr.coords[c0 * H * W:c1 * H * W], tr.sens_enc_B, save=False))
        x = sense_apply(img, sens[-1], c1 - c0, H, W, tr.sense_scale, 1)
        k = torch.fft.fftshift(torch.fft.fft2(torch.view_as_complex(x), norm="ortho"), dim=(-2, -1))
        want.append(torch.view_as_real(k).reshape(-1, 2))
    sens = torch.cat(sens, 0)
    assert got.shape == (tr.n, 2) and _bits(got, torch.cat(want, 0))
    # ... and the float64 composite of the trainer's CURRENT parameters, in the dataset's own order
    r64, r32 = Ref(tr, torch.float64), Ref(tr, torch.float32)
    with torch.no_grad():
        want, t32 = (Ref.kspace(r.i, r.s, r.Bi, r.Bs, r.img_coords, r.coords, r.scale, H, W).double().numpy()
                     for r in (r64, r32))
    e, e32 = rel_l2(got.cpu().numpy(), want), rel_l2(t32, want)
    print(f"predict_all vs the float64 composite: {e:.3e} (torch fp32 chain {e32:.3e})")
    assert e <= TOL, (e, e32)
    s = tr.sense_summary
    rss = torch.sqrt((sens.double() ** 2).view(C_, H * W, 2).sum(dim=(0, 2)))
    assert s["coils_per_step"] == len(range(*tr.groups[0])) and s["scale"] == tr.sense_scale
    assert s["net"] == {"width": 64, "depth": 3}
    for key, v in (("min", rss.min()), ("max", rss.max()), ("mean", rss.mean())):
        assert abs(s["sens_rss"][key] - float(v)) <= 1e-12 * float(v)
    rec = tr.validate(0)
    assert rec["sense"] == tr.sense_summary and tr.metrics()["sense"] == rec["sense"]
    assert rec["test_loss"] is not None and np.isfinite(rec["psnr"]) and np.isfinite(rec["ssim"])


def test_resume_is_bit_identical(dev):
    """coils_per_step = 2 of 3 coils (a short last group): 4 steps, checkpoint() into a new trainer through
    load_checkpoint, 2 more steps -- parameters, Adam moments and step count of both engines equal to the bit to those of
    6 uninterrupted steps"""
    whole, a, b = (_trainer(dev, coils_per_step=2) for _ in range(3))
    assert whole.groups == [(0, 2), (2, 3)]
    whole.fit(6)
    a.fit(4)
    ckpt = a.checkpoint()
    assert [k.split(".")[0] for k in ckpt["net"]] == ["image"] * 6 + ["sens"] * 6
    assert sorted(ckpt["opt"]["state"]) == list(range(12)) and ckpt["opt"]["param_groups"][0]["params"] == list(range(12))
    b.load_checkpoint(ckpt)
    assert b.engine.step == 4 and b.sens_engine.step == 4
    b.global_step = a.global_step  # fit() takes up the epoch loop where the checkpoint was written
    for epoch, it in ((2, 0), (2, 1)):
        b.step(epoch, it)
    for eb, ew in ((b.engine, whole.engine), (b.sens_engine, whole.sens_engine)):
        assert eb.step == ew.step == 6
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert _bits(getattr(eb, name), getattr(ew, name)), name


def test_reconstructor(dev, fit, tmp_path):
    """k-space of the native grid equals predict_all() bit for bit; the rendering itself is coil images; --scale 2 has the
    doubled shape and finite values; coils and window work"""
    from inr_mi355x.evalchain import ifft2c
    from inr_mi355x.reconstruct import Reconstructor
    tr = fit[0]
    path = str(tmp_path / "model.pt")
    ckpt = tr.checkpoint()
    assert [k.split(".")[0] for k in ckpt["net"]] == ["image"] * 6 + ["sens"] * 6
    assert sorted(ckpt["opt"]["state"]) == list(range(12)) and set(ckpt["sense"]) >= {"scale", "enc_B", "coils_per_step"}
    torch.save(ckpt, path)
    rec = Reconstructor(tr.config, path, shape=SHAPE, device=dev)
    assert rec.sens_model is not None and rec.sens_engine.exp_avg is None and rec.engine.exp_avg is None
    want = tr.predict_all()
    images = rec.render()
    assert images.shape == (*SHAPE, 2)
    got = rec.kspace(images)
    assert _bits(got.reshape(-1, 2), want), float((got.reshape(-1, 2) - want).abs().max())
    assert rel_l2(images.cpu().numpy(), ifft2c(want.view(*SHAPE, 2)).cpu().numpy()) <= TOL  # images, no FFT round trip
    assert rec.rss(images).shape == SHAPE[1:]
    fine = rec.render(scale=2)
    assert fine.shape == (3, 24, 20, 2) and bool(torch.isfinite(fine).all())
    sub = rec.render(coils=[1], window=(-0.5, 0.25, 0.1, 0.7), height=5, width=7)
    assert sub.shape == (1, 5, 7, 2) and bool(torch.isfinite(sub).all())
    one = rec.render(coils=[2])  # other rows per forward call than in a group: the forward tolerance of test_gpu_parity.py
    torch.testing.assert_close(one[0], images[2], rtol=1e-5, atol=1e-6)
    # resume: the same settings load, other settings are refused by name
    b = _trainer(dev, coils_per_step=tr.coils_per_step)
    b.load_checkpoint(ckpt)
    assert b.engine.step == 3 and b.sens_engine.step == 3 and _bits(b.engine.params, tr.engine.params)
    assert _bits(b.sens_engine.exp_avg_sq, tr.sens_engine.exp_avg_sq) and _bits(b.predict_all(), want)
    with pytest.raises(ValueError, match="scale"):
        _trainer(dev, coils_per_step=tr.coils_per_step, scale=0.5).load_checkpoint(ckpt)


def test_stash_budget_names_a_group_size_that_fits(dev):
    from inr_mi355x.train_sense import sens_net_params, sens_stash_bytes, sense_settings
    shape = (4, 64, 64)
    cfg = _cfg()
    params = sens_net_params(sense_settings(cfg, 4), cfg["encoder"])
    need = [sens_stash_bytes(params, True, 16, g * 64 * 64) for g in (1, 2, 3, 4)]
    assert need[0] < need[1] <= need[2] < need[3], need  # the budget below separates 2 coils from 4
    with pytest.raises(ValueError, match="max_stash_bytes") as e:
        _trainer(dev, shape=shape, max_stash_bytes=need[1])
    named = int(re.search(r"coils_per_step = (\d+)", str(e.value).split(";")[1]).group(1))
    assert 2 <= named < 4
    tr = _trainer(dev, shape=shape, max_stash_bytes=need[1], coils_per_step=named)
    assert tr.coils_per_step == named and len(tr.groups) == -(-4 // named)
    with pytest.raises(ValueError, match="not even"):
        _trainer(dev, shape=shape, max_stash_bytes=1)


def test_forty_steps_reduce_the_training_loss(dev):
    """4 x 16 x 12 under grid-3*2, all coils per step: the training loss after 40 steps is below the first step's, and the
    validation record carries ``sense`` with a finite sens_rss"""
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    shape = (4, 16, 12)
    tr = SenseFitTrainer(_cfg(max_epoch=40), make_kspace(*shape)[0], grid_coords(*shape, device=dev), shape, dev, seed=1)
    assert tr.steps_per_epoch == 1 and tr.coils_per_step == 4
    logged = tr.fit(40, log_every=1)
    assert len(logged) == 40 and tr.global_step == 40
    print("training loss, step 1 and step 40:", logged[0][1], logged[-1][1])
    assert np.isfinite(logged[-1][1]) and logged[-1][1] < logged[0][1]
    rec = tr.validate(39)
    assert all(np.isfinite(v) and v > 0 for v in rec["sense"]["sens_rss"].values())
    assert rec["sense"]["coils_per_step"] == 4 and np.isfinite(rec["psnr"])
