"""Off-grid SENSE fits on calibrated maps on the MI355X (``-m gpu``): the four entries of
csrc/inr_sense_nufft.hip / inr_nufft.hip's plain-layout forms against the composition of existing entries they replace
and against their fp32 numpy text, bit for bit; the two whole operators against float64 within the worst-case fp32
bounds of trajectory.nufft_error_bound / nufft_adjoint_error_bound with the product's roundings added; SenseFitTrainer
under ``sense.maps: calibrated`` + ``trajectory`` against float64 autograd.

Criteria: bit equality wherever the same arithmetic sees the same inputs.  The 8-byte-only views cover every operand on
whose alignment a path can depend and which its entry accepts so: img, maps, grid and dimg of prepare / finish (the
16-byte test of sense_pairs), val, pos and out of interp / spread.  Not misaligned: apod_y, apod_x and the spread's
weights, read by scalar 4-byte loads alone, and the grid of interp / spread, which those entries refuse below 16 bytes
as inr_nufft_interp / inr_nufft_spread do.  Operators: the gridding chain's bound
gamma(n) ... with n raised by the roundings the coil product adds in front of it (apply_one: a = sr*ir, re = a - b,
scale * re -- 3 on a component) or behind it (adjoint_one: ur = scale * v, f = sr * ur, tr = f + h -- 3 -- and one per
coil of the sum, G); gamma(n + k) <= gamma(n) (1 + k / n) (1 + 2^-20) for the n >= 45 and k <= 35 here, so the bound is scaled by
(n + k) / n with n the smallest rounding count either bound uses (45).  Step: 1e-5 relative on the loss and on the flat
gradient, the criterion of tests/test_gpu_sense_calib.py; each operator is compared with a float64 reference written with
the same operator (gridding: nufft_numpy's; exact: nudft_numpy's), so the gridding approximation's own error cancels.
Measured: loss 4.3e-7 / 6.0e-8 and gradient 9.7e-7 / 2.7e-7 under gridding / exact."""
import numpy as np
import pytest
import torch

import sense_nufft_cases as NC
from aux_bits_cases import dev as to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np_bits(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    return g.shape == want.shape and np.array_equal(g.view(np.int32), want.view(np.int32))


def _cx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1]


def _off8(a) -> torch.Tensor:
    """the array on the device behind a base pointer that is 8 but not 16-byte aligned"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    buf = torch.empty(a.size + 2, device="cuda", dtype=torch.from_numpy(a).dtype)
    view = buf[2:].view(*a.shape) if a.itemsize == 4 else buf[1:-1].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


@pytest.fixture(scope="module")
def cases(dev):
    """per shape, made once and left unchanged: the operands on the device, the apodisation, positions and bins"""
    from inr_mi355x import trajectory as T
    out = {}
    for (G, H, W) in NC.KERNEL_SHAPES:
        img, maps, grid, val, w = NC.operands(G, H, W)
        pos = NC.positions(H, W)
        out[(G, H, W)] = dict(img=img, maps=maps, grid=grid, val=val, w=w, pos=pos, d_img=to_dev(img), d_maps=to_dev(maps),
                              d_grid=to_dev(grid), d_val=to_dev(val), d_w=to_dev(w), d_pos=to_dev(pos),
                              apod=T.nufft_device_apodisation(H, W, dev), bins=T.nufft_device_bins(pos, H, W, dev))
    return out


# ---- the kernels against the composition they replace and against their fp32 text ------------------------------------------
@pytest.mark.parametrize("shape", NC.KERNEL_SHAPES, ids=NC.SHAPE_IDS)
def test_prepare_is_apply_then_prepare_rolled_and_its_numpy_text(dev, cases, shape):
    from inr_mi355x import _lib as L
    from inr_mi355x import sense_nufft as SN
    from inr_mi355x.sense import sense_apply
    G, H, W = shape
    c = cases[shape]
    got = SN.sense_nufft_prepare(c["d_img"], c["d_maps"], G, H, W, NC.SCALE, c["apod"],
                                 grid=torch.full((G, 2 * H, 2 * W, 2), float("nan"), device=dev))
    x = sense_apply(c["d_img"], c["d_maps"], G, H, W, NC.SCALE, 0)
    centred = torch.empty(G, 2 * H, 2 * W, 2, device=dev)
    L.launch("inr_nufft_prepare", dev, x.data_ptr(), c["apod"][0].data_ptr(), c["apod"][1].data_ptr(), G, H, W,
             centred.data_ptr())
    assert _bits(got, torch.roll(centred, (H, W), (1, 2))), shape
    assert _np_bits(got, SN.sense_nufft_prepare_numpy(c["img"], c["maps"], G, H, W, NC.SCALE)), shape
    # every operand behind an 8-byte-only base in turn, and all at once: the 8-byte path, the same bits
    ops = dict(img=c["d_img"], maps=c["d_maps"], grid=None)
    for which in ("img", "maps", "grid", "all"):
        a = {k: (_off8(v if v is not None else np.zeros((G, 2 * H, 2 * W, 2), np.float32))
                 if which in (k, "all") else v) for k, v in ops.items()}
        assert _bits(SN.sense_nufft_prepare(a["img"], a["maps"], G, H, W, NC.SCALE, c["apod"], grid=a["grid"]), got), which


@pytest.mark.parametrize("shape", NC.KERNEL_SHAPES, ids=NC.SHAPE_IDS)
def test_finish_is_finish_then_adjoint_and_its_numpy_text(dev, cases, shape):
    from inr_mi355x import _lib as L
    from inr_mi355x import sense_nufft as SN
    from inr_mi355x.sense_calib import sense_adjoint
    G, H, W = shape
    c = cases[shape]
    got = SN.sense_nufft_finish(c["d_grid"], c["d_maps"], G, H, W, NC.SCALE, c["apod"])
    centred = torch.roll(c["d_grid"], (H, W), (1, 2)).contiguous()
    coil = torch.empty(G, H, W, 2, device=dev)
    L.launch("inr_nufft_finish", dev, centred.data_ptr(), c["apod"][0].data_ptr(), c["apod"][1].data_ptr(), G, H, W,
             coil.data_ptr())
    want = sense_adjoint(c["d_maps"], coil, G, H, W, NC.SCALE, 0)
    assert _bits(got, want), shape
    assert _np_bits(got, SN.sense_nufft_finish_numpy(c["grid"], c["maps"], G, H, W, NC.SCALE)), shape
    assert _bits(SN.sense_nufft_finish(c["d_grid"], c["d_maps"], G, H, W, NC.SCALE, c["apod"]), got), "twice"
    # accumulate: the fp32 sum old + dI, in that order
    old = to_dev(NC.operands(G, H, W, seed=7)[0])
    acc = SN.sense_nufft_finish(c["d_grid"], c["d_maps"], G, H, W, NC.SCALE, c["apod"], dimg=old.clone(), accumulate=True)
    assert _bits(acc, old + want), "accumulate"
    assert _np_bits(acc, SN.sense_nufft_finish_numpy(c["grid"], c["maps"], G, H, W, NC.SCALE, dimg=old.cpu().numpy()))
    for which in ("grid", "maps", "dimg", "all"):
        g = _off8(c["d_grid"]) if which in ("grid", "all") else c["d_grid"]
        m = _off8(c["d_maps"]) if which in ("maps", "all") else c["d_maps"]
        for accumulate, ref in ((False, got), (True, acc)):
            d = _off8(old) if which in ("dimg", "all") else old.clone()
            assert _bits(SN.sense_nufft_finish(g, m, G, H, W, NC.SCALE, c["apod"], dimg=d, accumulate=accumulate), ref), which


@pytest.mark.parametrize("shape", NC.KERNEL_SHAPES, ids=NC.SHAPE_IDS)
def test_plain_interp_and_spread_equal_the_centred_entries(dev, cases, shape):
    from inr_mi355x import _lib as L
    from inr_mi355x import sense_nufft as SN
    from inr_mi355x import trajectory as T
    G, H, W = shape
    c = cases[shape]
    need = T.nufft_scratch_floats(G, H, W, NC.M)
    scratch = torch.empty(need, device=dev)
    # interp: the plain entry on the rolled grid gives what the centred entry gives on the grid itself
    want = torch.empty(G, NC.M, 2, device=dev)
    L.launch("inr_nufft_interp", dev, c["d_grid"].data_ptr(), c["d_pos"].data_ptr(), G, H, W, NC.M, want.data_ptr(),
             scratch.data_ptr(), need)
    rolled = torch.roll(c["d_grid"], (H, W), (1, 2)).contiguous()
    got = SN.nufft_interp_plain(rolled, c["d_pos"], G, H, W, scratch)
    assert _bits(got, want), shape
    assert _bits(SN.nufft_interp_plain(rolled, _off8(c["d_pos"]), G, H, W, scratch, out=_off8(got)), want), "8-byte views"
    # spread: the plain entry's grid is the centred entry's, rolled
    bin_start, order = c["bins"]
    for w in (None, c["d_w"]):
        centred = torch.empty(G, 2 * H, 2 * W, 2, device=dev)
        L.launch("inr_nufft_spread", dev, c["d_val"].data_ptr(), c["d_pos"].data_ptr(), None if w is None else w.data_ptr(),
                 bin_start.data_ptr(), order.data_ptr(), G, H, W, NC.M, centred.data_ptr(), scratch.data_ptr(), need)
        want_grid = torch.roll(centred, (H, W), (1, 2))
        grid = SN.nufft_spread_plain(c["d_val"], c["d_pos"], w, c["bins"], G, H, W, scratch,
                                     grid=torch.full((G, 2 * H, 2 * W, 2), float("nan"), device=dev))
        assert _bits(grid, want_grid), (shape, w is None)
        again = SN.nufft_spread_plain(_off8(c["d_val"]), _off8(c["d_pos"]), w, c["bins"], G, H, W, scratch)
        assert _bits(again, want_grid), "8-byte views"


def test_entries_refuse_bad_operands(dev, cases):
    from inr_mi355x import sense_nufft as SN
    G, H, W = NC.KERNEL_SHAPES[0]
    c = cases[(G, H, W)]
    with pytest.raises(RuntimeError, match="overlaps"):
        big = torch.zeros(G * 4 * H * W + H * W, 2, device=dev)
        SN.sense_nufft_prepare(big[:H * W], c["d_maps"], G, H, W, 1.0, c["apod"], grid=big[:G * 4 * H * W].view(G, 2 * H, 2 * W, 2))
    with pytest.raises(RuntimeError, match="scale"):
        SN.sense_nufft_prepare(c["d_img"], c["d_maps"], G, H, W, float("inf"), c["apod"])
    with pytest.raises(RuntimeError, match=">= 3"):
        SN.sense_nufft_prepare(torch.zeros(2 * 8, 2, device=dev), torch.zeros(2 * 8, 2, device=dev), 1, 2, 8, 1.0)
    with pytest.raises(RuntimeError, match="apod_y has shape"):
        SN.sense_nufft_finish(c["d_grid"], c["d_maps"], G, H, W, 1.0, (torch.zeros(H + 1, device=dev), c["apod"][1]))


# ---- the whole operators against float64 -------------------------------------------------------------------------------------
N_MIN = 45  # the smallest rounding count of the two gridding bounds: J^2 + 2 + 4 + 3 = 45 (forward, before the FFT's)
# fp32 roundings apply_one puts on a component of scale * S * I before the gridding chain sees it: a = sr*ir (1),
# re = a - b (2), scale * re (3)
PRODUCT_ROUNDINGS = 3


def adjoint_roundings(G: int) -> int:
    """fp32 roundings adjoint_one adds behind the gridding chain on a component of dI: ur = scale * v (1), f = sr * ur (2),
    tr = f + h (3), and one per addition of the coil sum (G)"""
    return 3 + G


def _raised(bound, extra: int):
    """the gridding bound with ``extra`` more roundings on every term (module docstring)"""
    return bound * (1.0 + extra / N_MIN) * (1.0 + 2.0 ** -20)


@pytest.mark.parametrize("shape", NC.KERNEL_SHAPES, ids=NC.SHAPE_IDS)
def test_operators_against_float64_within_the_rounding_bounds(dev, cases, shape):
    from inr_mi355x import sense_nufft as SN
    from inr_mi355x import trajectory as T
    G, H, W = shape
    c = cases[shape]
    S, I = _cx(c["maps"].reshape(G, H, W, 2)), _cx(c["img"].reshape(H, W, 2))
    # forward: the bound is evaluated on the float64 product images
    got = SN.sense_nufft(c["d_img"], c["d_maps"], c["pos"], G, H, W, NC.SCALE)
    want = SN.sense_nufft_numpy(c["img"], c["maps"], c["pos"], G, H, W, NC.SCALE)
    bound = _raised(T.nufft_error_bound(NC.SCALE * S * I[None], c["pos"]), PRODUCT_ROUNDINGS)
    err = np.abs(_cx(got.cpu().numpy()) - want)
    print("forward %s: max |out - ref| / bound = %.4f" % (shape, (err / bound[:, None]).max()))
    assert got.shape == (G, NC.M, 2) and (err <= bound[:, None]).all()
    # adjoint: every coil's back-gridded image within its bound, times |scale S_g|, summed over the coils
    for w in (None, c["w"]):
        got = SN.sense_nufft_adjoint(c["d_val"], c["d_maps"], c["pos"], (H, W), NC.SCALE, w)
        want = SN.sense_nufft_adjoint_numpy(c["val"], c["maps"], c["pos"], G, H, W, NC.SCALE, w)
        per_coil = _raised(T.nufft_adjoint_error_bound(c["val"], c["pos"], w, H, W), adjoint_roundings(G))
        bound = abs(NC.SCALE) * (np.abs(S) * per_coil[:, None, None]).sum(axis=0)
        # the roundings of adjoint_one and of the coil sum act on the values themselves as well
        back = np.abs(T.nufft_adjoint_numpy(c["val"], c["pos"], H, W, w))
        bound = bound + T._gamma(adjoint_roundings(G)) * abs(NC.SCALE) * (np.abs(S) * back).sum(axis=0)
        err = np.abs(_cx(got.cpu().numpy()).reshape(H, W) - want)
        print("adjoint %s %s: max |out - ref| / bound = %.4f" % (shape, "w null" if w is None else "weighted",
                                                                 (err / bound).max()))
        assert got.shape == (H * W, 2) and (err <= bound).all()


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
SHAPE = NC.FIT_SHAPE
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)


def _cfg(sense, **kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, max_epoch=10, weight_decay=0.0, beta1=0.9, beta2=0.999,
               trajectory=NC.FIT_TRAJECTORY, encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3),
               net=dict(NET), sense=sense)
    cfg.update(kw)
    return cfg


def _trainer(dev, seed=3, operator=None, **sense):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    sense = dict(dict(maps="calibrated", calib=dict(size=list(NC.FIT_BLOCK))), **sense)
    kw = {} if operator is None else dict(trajectory_operator=operator)
    return SenseFitTrainer(_cfg(sense, **kw), make_kspace(*SHAPE)[0], grid_coords(*SHAPE, device=dev), SHAPE, dev, seed=seed)


def _step_float64(tr, exact: bool):
    """(loss, flat gradient of the image network) of the trainer's first step in float64 on the host: the SIREN on the
    plane's rows with the coil column 0 (torch, for its autograd), E written with trajectory.nufft_numpy's operators
    (sense_nufft_numpy; ``exact``: nudft_numpy), the pointwise loss rows of gain.loss_rows_float64, E^H by the adjoint
    restatement (the conjugate transpose to 1e-12: tests/test_sense_nufft_host.py), back through the network"""
    import oracle as O  # checker only
    from inr_mi355x import sense_nufft as SN
    from inr_mi355x import trajectory as T
    from inr_mi355x.gain import loss_rows_float64
    C_, H, W = SHAPE
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in tr.model.state_dict().items()}
    coords = tr.coords[:tr.plane].cpu().double().clone()
    coords[:, 0] = 0
    I = O.siren_forward(p, O.encode(coords, tr.encoder.B.cpu().double(), "gauss"), NET)
    maps = _cx(tr._maps.cpu().double().numpy()).reshape(C_, H, W)
    Ic = _cx(I.detach().numpy()).reshape(H, W)
    gt = tr._gt.cpu().double().numpy()
    if exact:
        K = T.nudft_numpy(tr.sense_scale * maps * Ic[None], tr._pos)
    else:
        K = SN.sense_nufft_numpy(Ic, maps, tr._pos, C_, H, W, tr.sense_scale)
    Lr, g = loss_rows_float64(tr.loss, np.stack((K.real, K.imag), -1).reshape(-1, 2), gt, 1.0 / gt.shape[0], 0.0)
    gK = _cx(g).reshape(C_, -1)
    if exact:
        dI = tr.sense_scale * np.sum(np.conj(maps) * T.nudft_adjoint_numpy(gK, tr._pos, H, W), axis=0)
    else:
        dI = SN.sense_nufft_adjoint_numpy(gK, maps, tr._pos, C_, H, W, tr.sense_scale)
    I.backward(torch.from_numpy(np.stack((dI.real, dI.imag), -1).reshape(-1, 2)))
    return float(np.sum(Lr)), torch.cat([v.grad.reshape(-1) for v in p.values()]).numpy()


def _rel_l2(got, want):
    return float(np.linalg.norm(np.asarray(got).ravel() - np.asarray(want).ravel()) / np.linalg.norm(want))


@pytest.mark.parametrize("operator", ["gridding", "exact"])
def test_one_step_against_float64(dev, operator):
    """loss and the flat gradient of the image network after one step: 1e-5 relative, the criterion of
    tests/test_gpu_sense_calib.py::test_steps_against_float64 (fp32 kernels against float64 on a 3 x 32 SIREN)"""
    import sense_nufft_cases as cases
    from inr_mi355x import sense_calib as K
    tr = _trainer(dev, operator=None if operator == "gridding" else operator)
    assert tr.operator == operator and tr.groups == [(0, 3)] and tr.steps_per_epoch == 1 and tr.sens_model is None
    maps64, y, pos, w, block = cases.fit_samples()
    assert tr._gt.shape == (3 * pos.shape[0], 2) and np.array_equal(tr._pos, pos)
    assert _rel_l2(_cx(tr._gt.cpu().numpy()).reshape(3, -1), y) <= 1e-5  # the exact NUDFT's samples
    assert _rel_l2(tr._block.cpu().numpy(), block) <= 1e-5  # the block from the samples' own adjoint
    want_loss, want_g = _step_float64(tr, operator == "exact")
    loss = float(tr.step(0, 0))
    g = tr.engine.grads.cpu().numpy()
    errs = dict(loss=abs(loss - want_loss) / abs(want_loss), image=_rel_l2(g, want_g))
    print(f"off-grid SENSE step under {operator}: kernels vs float64 {errs}")
    assert np.linalg.norm(want_g) > 0 and errs["loss"] <= TOL and errs["image"] <= TOL, errs


def test_learned_maps_with_a_trajectory_still_raise(dev):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_sense import SenseFitTrainer
    with pytest.raises(NotImplementedError, match="trajectory"):
        SenseFitTrainer(_cfg(dict(net=dict(network_width=32, network_depth=3))), make_kspace(*SHAPE)[0],
                        grid_coords(*SHAPE, device=dev), SHAPE, dev, seed=3)


def test_cg_baseline_against_float64(dev):
    """cg-3 on the trainer's maps and samples: the last iterate within max(8 x the recorded host distance, 1e-5) of
    cg_sense_nufft_numpy on the same maps (the device's, widened) and samples; the record is scored and reported"""
    from inr_mi355x import sense_nufft as SN
    tr = _trainer(dev, baseline=f"cg-{NC.CG_ITERS}")
    C_, H, W = SHAPE
    cg = tr.cg_sense
    assert cg["iters"] == NC.CG_ITERS and cg["operator"] == "gridding" and len(cg["objective"]) == NC.CG_ITERS + 1
    assert np.isfinite(cg["psnr"]) and np.isfinite(cg["ssim"])
    maps = _cx(tr._maps.cpu().double().numpy()).reshape(C_, H, W)
    y = _cx(tr._gt.cpu().double().numpy()).reshape(C_, -1)
    want, want_obj = SN.cg_sense_nufft_numpy(maps, y, tr._pos, tr._op.weights.cpu().double().numpy(), NC.CG_ITERS)
    err = _rel_l2(_cx(tr._cg_image.cpu().numpy()).reshape(H, W), want[-1])
    tol = max(8 * NC.CG_FP32_REL_L2, NC.CG_FLOOR_TOL)
    print("non-Cartesian CG-SENSE last iterate vs float64:", err, "bound", tol, "objective", cg["objective"], want_obj)
    assert err <= tol
    assert all(abs(a - b) <= 1e-5 * want_obj[0] for a, b in zip(cg["objective"], want_obj))
    rec = tr.validate(0)
    assert rec["cg_sense"] == cg and rec["trajectory"]["kind"] == "spokes" and rec["sense"]["operator"] == "gridding"
    assert rec["sense"]["calib"]["source"] == "samples" and "acs" not in rec["sense"]["calib"]


def test_fit_checkpoint_resume_and_reconstructor(dev, tmp_path):
    from inr_mi355x.reconstruct import Reconstructor
    whole, a, b = (_trainer(dev) for _ in range(3))
    whole.fit(4)
    a.fit(2)  # two epochs: one step each
    ckpt = a.checkpoint()
    assert set(ckpt["sense"]) == {"scale", "coils_per_step", "maps", "calib", "block"}
    b.load_checkpoint(ckpt)
    for epoch in (2, 3):
        b.step(epoch, 0)
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert _bits(getattr(b.engine, name), getattr(whole.engine, name)), name
    path = str(tmp_path / "model.pt")
    torch.save(whole.checkpoint(), path)
    rec = Reconstructor(whole.config, path, shape=SHAPE, device=dev)
    images = rec.render()
    assert images.shape == (*SHAPE, 2) and bool(torch.isfinite(images).all())
    assert _bits(rec.kspace(images).reshape(-1, 2), whole.predict_all())
