"""SENSE fits on calibrated coil maps on the MI355X (``-m gpu``): inr_sense_lowres / inr_sense_maps /
inr_sense_adjoint against the fp32 numpy text of inr_mi355x/sense_calib.py bit for bit, and SenseFitTrainer /
Reconstructor / CG-SENSE under ``sense.maps: calibrated`` against float64.

Criteria -- none of them new: bit equality wherever the same arithmetic sees the same inputs; 1e-5 relative L2 per array
and 1e-5 relative on the loss against float64; parameters after three steps as tests/test_gpu_sense.py compares them
(relative L2 of the flat vector below 5e-5).  CG-SENSE: 8 x the distance of the fp32 numpy operators from float64 on the
same inputs (sense_calib_cases.CG_FP32_REL_L2, measured on the host), never less than 1e-5."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import oracle as O  # checker only
import sense_calib_cases as CC
from aux_bits_cases import _stream, dev as to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_PARAMS = 5e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rel_l2(got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.abs(got).max(initial=0.0))


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np_bits(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    return g.shape == want.shape and np.array_equal(g.view(np.int32), want.view(np.int32))


def _cx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1]


def _off8(a: np.ndarray) -> torch.Tensor:
    """the array on the device behind a base pointer that is 8 but not 16-byte aligned"""
    buf = torch.empty(a.size + 2, device="cuda")
    view = buf[2:].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


# ---- the kernels against their fp32 text -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.CASE_IDS)
def test_lowres_and_maps_equal_the_fp32_text_bit_for_bit(dev, case):
    """native grid; floor 0 and a floor that removes pixels; a second call gives the same bits; views that are 8 but not
    16-byte aligned give the aligned result"""
    from inr_mi355x import sense_calib as K
    (C, H, W), (a, b) = case
    block = K.cut_block(CC.kspace(C, H, W), a, b, "hann")
    ey, ex = K.grid_tables(H, W, a, b)
    want_low = K.lowres_numpy(block, ey, ex)
    d_block, d_ey, d_ex = to_dev(block), to_dev(ey), to_dev(ex)
    low = K.sense_lowres(d_block, d_ey, d_ex)
    torch.cuda.synchronize()
    assert _np_bits(low, want_low), (case, "low")
    assert _bits(K.sense_lowres(d_block, d_ey, d_ex), low), (case, "low twice")
    assert _bits(K.sense_lowres(_off8(block), _off8(ey), _off8(ex), out=_off8(np.zeros_like(want_low))), low)
    P = H * W
    for floor in CC.FLOORS:
        want_maps, want_rss = K.maps_numpy(want_low, C, P, floor)
        maps, rss = K.sense_maps(low, C, P, floor)
        torch.cuda.synchronize()
        assert _np_bits(rss, want_rss), (case, floor, "rss")
        assert _np_bits(maps, want_maps), (case, floor, "maps")
        if floor > 0:
            assert 0 < int((want_rss > np.float32(floor) * want_rss.max()).sum()) < P  # the floor removes some pixels, not all
        m2, r2 = K.sense_maps(low, C, P, floor)
        assert _bits(m2, maps) and _bits(r2, rss), (case, floor, "twice")
        m3, r3 = K.sense_maps(_off8(want_low), C, P, floor, maps=_off8(np.zeros_like(want_maps)))
        assert _bits(m3, maps) and _bits(r3, rss), (case, floor, "misaligned")


@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.CASE_IDS)
def test_adjoint_equals_its_text_and_the_dimg_of_sense_grad(dev, case):
    """shift 0 and 1; a second call; misaligned views; and inr_sense_grad's dimg on the same inputs, bit for bit"""
    from inr_mi355x import sense as S
    from inr_mi355x import sense_calib as K
    (G, H, W), _ = case
    sens, gx, img = CC.adjoint_inputs(G, H, W)
    ds, dg, di = to_dev(sens), to_dev(gx), to_dev(img)
    assert all(t.data_ptr() % 16 == 0 for t in (ds, dg, di))
    for shift in (0, 1):
        dimg = K.sense_adjoint(ds, dg, G, H, W, CC.SCALE, shift)
        torch.cuda.synchronize()
        assert _np_bits(dimg, K.sense_adjoint_numpy(sens, gx, G, H, W, CC.SCALE, shift)), (case, shift)
        assert _bits(K.sense_adjoint(ds, dg, G, H, W, CC.SCALE, shift), dimg), (case, shift, "twice")
        assert _bits(S.sense_grad(di, ds, dg, G, H, W, CC.SCALE, shift)[0], dimg), (case, shift, "inr_sense_grad")
        assert _bits(K.sense_adjoint(_off8(sens), _off8(gx), G, H, W, CC.SCALE, shift), dimg), (case, shift, "off8 in")
        out = _off8(np.zeros((H * W, 2), np.float32))
        assert _bits(K.sense_adjoint(ds, dg, G, H, W, CC.SCALE, shift, dimg=out), dimg), (case, shift, "off8 out")


@pytest.mark.parametrize("case", CC.KERNEL_CASES[:4], ids=CC.CASE_IDS[:4])
def test_lowres_on_other_grids(dev, case):
    """a 2x grid and an off-centre window: the fp32 text bit for bit, and the float64 statement at 1e-5"""
    from inr_mi355x import sense_calib as K
    (C, H, W), (a, b) = case
    block = K.cut_block(CC.kspace(C, H, W), a, b, "hann")
    for Ho, Wo, window in ((2 * H, 2 * W, K.FULL_WINDOW), (5, 7, (-0.5, 0.25, 0.1, 0.7))):
        ey, ex = K.grid_tables(H, W, a, b, Ho, Wo, window)
        low = K.sense_lowres(to_dev(block), to_dev(ey), to_dev(ex))
        assert _np_bits(low, K.lowres_numpy(block, ey, ex)), (case, Ho, Wo)
        ey64 = K.phasor_table_float64(K.block_index(H, a), K.axis_positions(H, Ho, *window[:2]), H)
        ex64 = K.phasor_table_float64(K.block_index(W, b), K.axis_positions(W, Wo, *window[2:]), W)
        e = rel_l2(_cx(low.cpu().numpy()), K.lowres_float64(block, ey64, ex64))
        print(case, (Ho, Wo), "lowres vs float64:", e)
        assert e <= TOL
        maps, rss = K.calibrate(to_dev(block), H, W, 0.0, Ho, Wo, window)
        m64, r64 = K.calibrate_numpy(block, H, W, 0.0, Ho, Wo, window)
        assert rel_l2(_cx(maps.cpu().numpy()).reshape(C, Ho, Wo), m64) <= TOL and rel_l2(rss.cpu().numpy(), r64) <= TOL


def test_bad_arguments_leave_the_outputs_alone(dev):
    """host-side argument checks only: every call returns INR_ERR_INVALID (-1) before any launch"""
    from inr_mi355x import _lib as L
    from inr_mi355x import sense_calib as K
    lib = L.load()
    C, H, W, a, b = 2, 4, 6, 3, 2
    block = to_dev(K.cut_block(CC.kspace(C, H, W), a, b, "hann"))
    ey, ex = (to_dev(t) for t in K.grid_tables(H, W, a, b))
    sens, gx, _ = (to_dev(t) for t in CC.adjoint_inputs(C, H, W))
    sent = 123.25
    low, maps, rss, dimg = (torch.full(s, sent, device=dev) for s in ((C, H, W, 2), (C, H * W, 2), (H * W,), (H * W, 2)))
    lowin = to_dev(CC.kspace(C, H, W))
    p = lambda t: t.data_ptr()
    st = _stream()
    f = Ct.c_float

    def swap(ok, i, v):
        return ok[:i] + [v] + ok[i + 1:]

    ok_l = [p(block), p(ey), p(ex), C, a, b, H, W, p(low)]
    bad_l = [swap(ok_l, i, None) for i in (0, 1, 2, 8)] + [swap(ok_l, i, ok_l[i] + 4) for i in (0, 1, 2, 8)]
    bad_l += [swap(ok_l, 3, v) for v in (0, -1, 65536)] + [swap(ok_l, 4, v) for v in (1, 0, 65, -2)]
    bad_l += [swap(ok_l, 5, v) for v in (1, 65)] + [swap(ok_l, 6, v) for v in (0, -1, (1 << 20) + 1)]
    bad_l += [swap(ok_l, 7, v) for v in (0, (1 << 20) + 1)]
    bad_l += [[p(block), p(ey), p(ex), 4, a, b, 1 << 20, 1 << 19, p(low)]]  # more than 2^40 complex numbers
    bad_l += [swap(ok_l, 8, p(block)), swap(ok_l, 8, p(ey)), swap(ok_l, 8, p(ex))]  # overlap
    for args in bad_l:
        assert lib.inr_sense_lowres(*args, st) == -1, args
        assert "inr_sense_lowres" in L.last_error()
    assert lib.inr_sense_lowres(*swap(ok_l, 8, p(ex)), st) == -1 and "overlaps" in L.last_error()

    ok_m = [p(lowin), C, H * W, f(0.0), p(maps), p(rss)]
    bad_m = [swap(ok_m, i, None) for i in (0, 4, 5)] + [swap(ok_m, i, ok_m[i] + 4) for i in (0, 4)]
    bad_m += [swap(ok_m, 5, p(rss) + 2), swap(ok_m, 1, 0), swap(ok_m, 2, 0), swap(ok_m, 2, (1 << 40) + 1)]
    bad_m += [swap(ok_m, 3, f(v)) for v in (-0.5, 1.0, float("nan"), float("inf"))]
    bad_m += [swap(ok_m, 4, p(lowin)), swap(ok_m, 5, p(lowin)), swap(ok_m, 5, p(maps))]
    for args in bad_m:
        assert lib.inr_sense_maps(*args, st) == -1, args
        assert "inr_sense_maps" in L.last_error()

    ok_a = [p(sens), p(gx), C, H, W, f(0.5), 1, p(dimg)]
    bad_a = [swap(ok_a, i, None) for i in (0, 1, 7)] + [swap(ok_a, i, ok_a[i] + 4) for i in (0, 1, 7)]
    bad_a += [swap(ok_a, i, v) for i in (2, 3, 4) for v in (0, -1)]
    bad_a += [swap(ok_a, 5, f(v)) for v in (float("inf"), float("nan"))] + [swap(ok_a, 6, v) for v in (2, -1)]
    bad_a += [swap(ok_a, 3, (1 << 30) + 1), [p(sens), p(gx), 4, 1 << 20, 1 << 19, f(0.5), 1, p(dimg)]]
    bad_a += [swap(ok_a, 7, p(sens)), swap(ok_a, 7, p(gx) + 8)]
    for args in bad_a:
        assert lib.inr_sense_adjoint(*args, st) == -1, args
        assert "inr_sense_adjoint" in L.last_error()
    torch.cuda.synchronize()
    for buf in (low, maps, rss, dimg):
        assert bool((buf == sent).all())
    assert _np_bits(sens, CC.adjoint_inputs(C, H, W)[0]) and _np_bits(gx, CC.adjoint_inputs(C, H, W)[1])
    assert _np_bits(lowin, CC.kspace(C, H, W))


# ---- the trainer -------------------------------------------------------------------------------------------------------
SHAPE = CC.FIT_SHAPE
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)


def _cfg(sense, **kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, max_epoch=10, weight_decay=0.0, beta1=0.9, beta2=0.999,
               undersampling="grid-3*2", encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(NET))
    if sense is not None:
        cfg["sense"] = sense
    cfg.update(kw)
    return cfg


def _trainer(dev, seed=3, **sense):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    C_, H, W = SHAPE
    sense = dict(dict(maps="calibrated", calib=dict(size=list(CC.FIT_BLOCK))), **sense)
    return SenseFitTrainer(_cfg(sense), make_kspace(C_, H, W)[0], grid_coords(C_, H, W, device=dev), SHAPE, dev, seed=seed)


class Ref64:
    """the step in float64 on the host: the SIREN image network on the plane's rows with the coil column 0 (torch, for
    its autograd), then sense.sense_chain_numpy with the trainer's calibrated maps -- loss and dI -- back through the
    network, and stock torch.optim.Adam with the trainer's per-epoch learning rate"""

    def __init__(self, tr):
        self.p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in tr.model.state_dict().items()}
        self.B = tr.encoder.B.cpu().double()
        self.cfg = tr.config
        self.opt = torch.optim.Adam(list(self.p.values()), lr=self.cfg["lr"], betas=(self.cfg["beta1"], self.cfg["beta2"]),
                                    weight_decay=self.cfg["weight_decay"])
        self.img_coords = tr.coords[:tr.plane].cpu().double().clone()
        self.img_coords[:, 0] = 0
        self.gt = tr.image_full.cpu().double().numpy()
        self.mask = tr.mask_cpu.reshape(-1).numpy() != 0
        self.maps = tr._maps.cpu().double().numpy().reshape(-1, 2)
        self.scale, self.loss = tr.sense_scale, tr.loss

    def image(self):
        return O.siren_forward(self.p, O.encode(self.img_coords, self.B, "gauss"), NET)

    def step(self, epoch):
        from inr_mi355x.sense import sense_chain_numpy
        C_, H, W = SHAPE
        for g in self.opt.param_groups:
            g["lr"] = self.cfg["lr"] * 0.2 ** min(epoch / self.cfg["max_epoch"], 1)
        I = self.image()
        loss, dimg, _ = sense_chain_numpy(I.detach().numpy(), self.maps, self.gt, self.mask, self.loss, int(self.mask.sum()),
                                          C_, H, W, self.scale)
        self.opt.zero_grad()
        I.backward(torch.from_numpy(dimg))
        grads = torch.cat([p.grad.reshape(-1) for p in self.p.values()]).numpy().copy()
        self.opt.step()
        return loss, grads

    def params(self):
        return torch.cat([v.detach().reshape(-1) for v in self.p.values()]).numpy()


@pytest.fixture(scope="module")
def fit(dev):
    """(trainer after 3 steps, the float64 reference after the same steps, what each step gave)"""
    tr = _trainer(dev)
    assert tr.groups == [(0, 3)] and tr.steps_per_epoch == 1 and tr.sens_model is None and tr.sens_engine is None
    ref = Ref64(tr)
    seen = []
    for epoch in range(3):
        loss = float(tr.step(epoch, 0))
        seen.append((loss, tr.engine.grads.cpu().numpy().copy(), ref.step(epoch)))
    return tr, ref, seen


def test_ingest_masks_and_maps(dev, fit):
    from inr_mi355x import sense_calib as K
    tr = fit[0]
    C_, H, W = SHAPE
    maps64, y, mask, block = CC.fit_problem()
    assert np.array_equal(tr.mask_cpu.numpy().reshape(C_, H, W) != 0, mask)  # grid-3*2 with the 4 x 4 block OR-ed in
    assert tr.acceleration == mask.size / mask.sum()
    assert _np_bits(tr._block, block)
    want_maps, want_rss = K.calibrate_numpy(block, H, W, fp32=True)
    assert _np_bits(tr._maps, want_maps) and _np_bits(tr.sens_rss, want_rss)
    assert bool((tr.image.view(C_, H, W, 2)[torch.from_numpy(~mask).to(dev)] == 0).all())  # zero-filled outside the mask


def test_steps_against_float64(fit):
    """loss and the flat gradient of the image network, steps 1 and 2: 1e-5 relative"""
    _, _, seen = fit
    for n, (loss, g, (l64, g64)) in enumerate(seen[:2]):
        errs = dict(loss=abs(loss - l64) / abs(l64), image=rel_l2(g, g64))
        print(f"step {n + 1}: kernels vs float64 {errs}")
        assert np.linalg.norm(g64) > 0
        for k, v in errs.items():
            assert v <= TOL, (n, k, v)


def test_three_steps_against_float64_adam(fit):
    tr, ref, _ = fit
    assert tr.engine.step == 3 and tr.global_step == 3
    got, want = tr.engine.params.cpu().numpy(), ref.params()
    e = rel_l2(got, want)
    print(f"params after 3 steps: rel L2 {e:.3e}, largest entry difference {np.abs(got - want).max():.3e}")
    assert got.shape == want.shape and e < TOL_PARAMS, e


def test_predict_raw_is_the_hand_run_sweep_and_the_record_says_so(dev, fit):
    from inr_mi355x.sense import sense_apply
    tr = fit[0]
    C_, H, W = SHAPE
    got = tr._predict_raw()
    img = tr.engine.forward(tr._img_in, tr.enc_B, save=False)
    x = sense_apply(img, tr._maps.view(-1, 2), C_, H, W, tr.sense_scale, 1)
    k = torch.fft.fftshift(torch.fft.fft2(torch.view_as_complex(x), norm="ortho"), dim=(-2, -1))
    assert got.shape == (tr.n, 2) and _bits(got, torch.view_as_real(k).reshape(-1, 2))
    s = tr.sense_summary
    assert s["maps"] == "calibrated" and "net" not in s and s["coils_per_step"] == 3 and s["scale"] == tr.sense_scale
    assert s["calib"] == {"size": [4, 4], "window": "hann", "floor": 0.0, "acs": True, "acceleration": tr.acceleration}
    rss = tr.sens_rss.double()
    assert s["sens_rss"]["min"] == float(rss.min()) and s["sens_rss"]["max"] == float(rss.max())
    assert abs(s["sens_rss"]["mean"] - float(rss.mean())) <= 1e-6 * float(rss.mean())
    rec = tr.validate(0)
    assert rec["sense"] == tr.sense_summary and tr.metrics()["sense"] == rec["sense"] and "cg_sense" not in rec
    assert rec["test_loss"] is not None and np.isfinite(rec["psnr"]) and np.isfinite(rec["ssim"])


def test_baseline_leaves_the_fit_alone_and_is_reported(dev, fit, tmp_path):
    tr = fit[0]
    b = _trainer(dev, baseline=f"cg-{CC.CG_ITERS}")
    for epoch in range(3):
        b.step(epoch, 0)
    assert _bits(b.engine.params, tr.engine.params) and _bits(b.engine.exp_avg_sq, tr.engine.exp_avg_sq)
    cg = b.cg_sense
    assert set(cg) == {"iters", "lambda", "psnr", "ssim", "objective", "seconds"}
    assert cg["iters"] == CC.CG_ITERS and cg["lambda"] == 0.0 and len(cg["objective"]) == CC.CG_ITERS + 1
    assert np.isfinite(cg["psnr"]) and np.isfinite(cg["ssim"]) and cg["seconds"] >= 0
    rec = b.validate(0)
    assert rec["cg_sense"] == cg and b.metrics()["cg_sense"] == cg
    # scored as the fit's prediction is: the k-space of the CG image through the validation's metric path
    from inr_mi355x.sense_calib import kspace_of
    m = b._device_metrics(b.image_full, kspace_of(b._cg_image, b._maps, SHAPE), False)
    assert m[:2].cpu().tolist() == [cg["psnr"], cg["ssim"]]
    path = b.save_cg_sense_image(str(tmp_path))
    assert path.endswith("cg_sense_{:.4g}_psnr_{:.4g}_ssim.png".format(cg["psnr"], cg["ssim"]))
    with pytest.raises(RuntimeError, match="baseline"):
        tr.save_cg_sense_image(str(tmp_path))


def test_cg_sense_against_float64(dev, fit):
    """3 iterations on the trainer's maps, samples and mask: the last iterate within max(8 x the recorded distance of the
    fp32 numpy operators from float64, 1e-5) of cg_sense_numpy, and an objective that does not increase"""
    from inr_mi355x import sense_calib as K
    tr = fit[0]
    maps64, y, mask, _ = CC.fit_problem()
    assert _np_bits(tr._maps.view(*SHAPE, 2), np.stack((maps64.real, maps64.imag), -1).astype(np.float32))
    iterates, objective = K.cg_sense(tr._maps, tr._gt_s, tr._mask_s, SHAPE, CC.CG_ITERS)
    want, want_obj = K.cg_sense_numpy(maps64, y, mask, CC.CG_ITERS)
    tol = max(8 * CC.CG_FP32_REL_L2, CC.CG_FLOOR_TOL)
    errs = [rel_l2(_cx(g.cpu().numpy()).reshape(SHAPE[1:]), w) for g, w in zip(iterates, want)]
    print("CG-SENSE iterates vs float64:", errs, "bound", tol, "objective", objective, "float64", want_obj)
    assert len(iterates) == CC.CG_ITERS and errs[-1] <= tol, (errs, tol)
    assert all(b_ <= a_ for a_, b_ in zip(objective, objective[1:])), objective
    assert all(abs(a_ - b_) <= 1e-5 * want_obj[0] for a_, b_ in zip(objective, want_obj))


def test_resume_is_bit_identical(dev):
    """one part under 'image.': 4 steps, checkpoint() into a new trainer through load_checkpoint, 2 more steps --
    parameters, Adam moments and step count equal to the bit to those of 6 uninterrupted steps"""
    whole, a, b = (_trainer(dev) for _ in range(3))
    whole.fit(6)
    a.fit(4)
    ckpt = a.checkpoint()
    assert all(k.startswith("image.") for k in ckpt["net"]) and len(ckpt["net"]) == 6
    assert sorted(ckpt["opt"]["state"]) == list(range(6)) and ckpt["opt"]["param_groups"][0]["params"] == list(range(6))
    b.load_checkpoint(ckpt)
    assert b.engine.step == 4
    for epoch in (4, 5):  # one group: one step per epoch
        b.step(epoch, 0)
    assert b.engine.step == whole.engine.step == 6
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert _bits(getattr(b.engine, name), getattr(whole.engine, name)), name


def test_reconstructor_round_trip(dev, fit, tmp_path):
    from inr_mi355x.reconstruct import Reconstructor
    tr = fit[0]
    ckpt = tr.checkpoint()
    assert all(k.startswith("image.") for k in ckpt["net"]) and len(ckpt["net"]) == 6
    assert set(ckpt["sense"]) == {"scale", "coils_per_step", "maps", "calib", "block"}
    assert tuple(ckpt["sense"]["block"].shape) == (3, 4, 4, 2) and not ckpt["sense"]["block"].is_cuda
    path = str(tmp_path / "model.pt")
    torch.save(ckpt, path)
    rec = Reconstructor(tr.config, path, shape=SHAPE, device=dev)
    assert rec.sens_model is None and rec.sense_block is not None and rec.engine.exp_avg is None
    want = tr.predict_all()
    images = rec.render()
    assert images.shape == (*SHAPE, 2)
    got = rec.kspace(images)
    assert _bits(got.reshape(-1, 2), want), float((got.reshape(-1, 2) - want).abs().max())
    assert rec.rss(images).shape == SHAPE[1:]
    cmp_ = rec.compare(images, tr.image_full)
    assert np.isfinite(cmp_["psnr"]) and np.isfinite(cmp_["ssim"])
    fine = rec.render(scale=2)
    assert fine.shape == (3, 24, 20, 2) and bool(torch.isfinite(fine).all())
    sub = rec.render(coils=[1], window=(-0.5, 0.25, 0.1, 0.7), height=5, width=7)
    assert sub.shape == (1, 5, 7, 2) and bool(torch.isfinite(sub).all())
    one = rec.render(coils=[2])  # the maps' RSS is over ALL coils, whichever are rendered
    assert _bits(one[0], images[2])
    # resume: the same settings load; another mode, calibration or data is refused by name
    b = _trainer(dev)
    b.load_checkpoint(ckpt)
    assert b.engine.step == 3 and _bits(b.engine.params, tr.engine.params) and _bits(b.predict_all(), want)
    with pytest.raises(ValueError, match="calib"):
        _trainer(dev, calib=dict(size=list(CC.FIT_BLOCK), window="none")).load_checkpoint(ckpt)
    with pytest.raises(ValueError, match="scale"):
        _trainer(dev, scale=0.5).load_checkpoint(ckpt)
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    learned = SenseFitTrainer(_cfg(dict(net=dict(network_width=32, network_depth=3))), make_kspace(*SHAPE)[0],
                              grid_coords(*SHAPE, device=dev), SHAPE, dev, seed=3)
    with pytest.raises(ValueError, match="maps = 'calibrated'"):
        learned.load_checkpoint(ckpt)
    with pytest.raises(ValueError, match="maps = 'learned'"):
        b.load_checkpoint(learned.checkpoint())


def test_acs_false_needs_the_block_in_the_mask(dev):
    with pytest.raises(ValueError, match=r"not fully sampled.*: \d+ of its 48 entries"):
        _trainer(dev, calib=dict(size=list(CC.FIT_BLOCK), acs=False))


def test_learned_maps_step_is_the_same_with_and_without_the_key(dev):
    """maps: learned is today's fit: the loss bits and the parameters of both networks after one step, with the key
    spelled and with it absent"""
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    out = []
    for sense in (dict(net=dict(network_width=32, network_depth=3)),
                  dict(net=dict(network_width=32, network_depth=3), maps="learned")):
        tr = SenseFitTrainer(_cfg(sense), make_kspace(*SHAPE)[0], grid_coords(*SHAPE, device=dev), SHAPE, dev, seed=3)
        assert tr.calib is None and tr.sens_engine is not None
        loss = tr.step(0, 0).reshape(1).clone()
        out.append((loss, tr.engine.params.clone(), tr.sens_engine.params.clone(), tr.sense_scale))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][1], out[1][1]) and _bits(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] and np.isfinite(float(out[0][0]))
