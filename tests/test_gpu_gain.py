"""Learned radial gain on the MI355X (``-m gpu``): inr_gain_loss_grad / inr_gain_apply against the
float64 statement of inr_mi355x/gain.py, the gain network's default plan (FFN 2 -> 512 x 8 -> 1) against float64, and
ScaledFitTrainer / Reconstructor against torch float64 autograd of the composite res = backbone(x) exp(-scaler(z)).

Criteria -- none of them new: 1e-5 relative L2 per array and 1e-5 relative on the loss against float64 (the plain
criterion of tests/test_gpu_matrix.py); parameters after three steps as tests/test_gpu_configs.py::
test_config1_siren_image_space compares them (relative L2 of the flat vector below 5e-5); bit equality wherever the
same kernels see the same inputs."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import loss_cases as C
import oracle as O  # checker only
from aux_bits_cases import _stream, dev as to_dev, rnd

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 255, 256, 257, 16385)  # empty blocks, the per-block partition edges, one row past 64 x 256
MASKS = ("none", "random", "ones", "zeros")
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _spec(kind):
    from inr_mi355x.engine import LossSpec
    return LossSpec(C.KINDS[kind], C.EPS, 2.0, C.FACTOR, 3000)


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.abs(got).max(initial=0.0))


def _rows(kind, B):
    """y, gt at amplitude 0.3 (msle: positive), s uniform in [-3, 3]: the sigmoid only gives (0, 1), the kernel must not
    rely on that"""
    y, t = rnd(B * 2, 31, 0.3).reshape(B, 2), rnd(B * 2, 32, 0.3).reshape(B, 2)
    if kind == "msle":
        y, t = np.abs(y) + np.float32(0.05), np.abs(t) + np.float32(0.05)
    return y, rnd(B, 33, 3.0), t


def _mask(tag, B):
    if tag == "none":
        return None, B
    if tag == "random":
        m = (rnd(B, 34) > 0).astype(np.uint8)
        m[0] = 1
        return m, int(m.sum())
    if tag == "ones":
        return np.ones(B, dtype=np.uint8), B
    return np.zeros(B, dtype=np.uint8), 1  # nothing sampled, count = 1


def _call(kind, y, s, t, m, count, want_res=True, hdr_A=C.HDR_A):
    from inr_mi355x import gain as G
    loss, res, dy, ds = G.gain_loss_grad(_spec(kind), y, s, t, count, mask=m, hdr_A=hdr_A, want_res=want_res)
    torch.cuda.synchronize()
    return loss.clone(), res, dy, ds


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel against the float64 statement --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(C.KINDS))
def test_kernel_against_float64(dev, kind):
    """every size and mask: loss, res, dy, ds at 1e-5; an all-zero mask gives loss 0 and dy = ds = 0 exactly; res = NULL
    and a second call give the same bits; inr_gain_apply equals res bit for bit, in place too"""
    from inr_mi355x import gain as G
    worst = {}
    for B in SIZES:
        y, s, t = _rows(kind, B)
        yd, sd, td = to_dev(y), to_dev(s), to_dev(t)
        for tag in MASKS:
            m, count = _mask(tag, B)
            md = None if m is None else to_dev(m)
            ref = G.gain_loss_grad_numpy(_spec(kind), y, s, t, m, count, C.HDR_A)
            loss, res, dy, ds = _call(kind, yd, sd, td, md, count)
            got = (float(loss), res.cpu().numpy(), dy.cpu().numpy(), ds.cpu().numpy())
            assert all(np.all(np.isfinite(g)) for g in got), (kind, B, tag)
            errs = dict(loss=abs(got[0] - ref[0]) / abs(ref[0]) if ref[0] != 0 else abs(got[0]),
                        res=rel_l2(got[1], ref[1]), dy=rel_l2(got[2], ref[2]), ds=rel_l2(got[3], ref[3]))
            print(kind, B, tag, {k: f"{v:.2e}" for k, v in errs.items()})
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= TOL, (kind, B, tag, k, v)
            if m is not None:
                assert not got[2][m == 0].any() and not got[3][m == 0].any(), (kind, B, tag, "an unsampled row is not 0")
            if tag == "zeros":
                assert got[0] == 0.0 and not got[2].any() and not got[3].any()
            loss2, none, dy2, ds2 = _call(kind, yd, sd, td, md, count, want_res=False)
            assert none is None and _bits(loss2, loss) and _bits(dy2, dy) and _bits(ds2, ds), (kind, B, tag, "res = NULL")
            loss3, res3, dy3, ds3 = _call(kind, yd, sd, td, md, count)
            assert _bits(loss3, loss) and _bits(res3, res) and _bits(dy3, dy) and _bits(ds3, ds), (kind, B, tag, "twice")
        assert _bits(G.gain_apply(yd, sd), res)
        inplace = yd.clone()
        assert G.gain_apply(inplace, sd, out=inplace) is inplace and _bits(inplace, res)
    from conftest import record_parity
    record_parity("gain:kernel/" + kind, **worst)


def test_alignment_changes_no_bit(dev):
    """views that start one row into a buffer (8-byte aligned y / gt, 4-byte aligned s): the narrow accesses give the bits
    of the wide ones"""
    from inr_mi355x import gain as G
    B = 777
    y, s, t = _rows("hdr", B + 1)
    m, _ = _mask("random", B + 1)
    yd, sd, td, md = to_dev(y), to_dev(s), to_dev(t), to_dev(m)
    count = int(m[1:].sum())
    a = _call("hdr", yd[1:].clone(), sd[1:].clone(), td[1:].clone(), md[1:].clone(), count)
    assert yd[1:].data_ptr() % 16 == 8
    b = _call("hdr", yd[1:], sd[1:], td[1:], md[1:], count)
    assert all(_bits(p, q) for p, q in zip(a, b))
    assert _bits(G.gain_apply(yd[1:], sd[1:]), a[1])


def test_bad_arguments_leave_the_outputs_alone(dev):
    from inr_mi355x import _lib as L
    lib = L.load()
    B = 64
    y, s, t = (to_dev(a) for a in _rows("l2", B))
    sent = 123.25
    res, dy = torch.full((B, 2), sent, device=dev), torch.full((B, 2), sent, device=dev)
    ds, loss = torch.full((B,), sent, device=dev), torch.full((L.LOSS_WORDS,), sent, device=dev)
    ld = L.LossDesc(kind=0, eps=1e-3, sigma=2.0, factor=0.5, inv_count=1.0 / B, hdr_A=0.0)
    bad_kind = L.LossDesc(kind=7, inv_count=1.0)
    p = lambda x: x.data_ptr()
    st = _stream()
    calls = [
        (None, p(y), p(s), p(t), None, B, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(ld), None, p(s), p(t), None, B, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(ld), p(y), None, p(t), None, B, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(ld), p(y), p(s), None, None, B, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(ld), p(y), p(s), p(t), None, B, p(res), None, p(dy), p(ds)),
        (Ct.byref(ld), p(y), p(s), p(t), None, B, p(res), p(loss), None, p(ds)),
        (Ct.byref(ld), p(y), p(s), p(t), None, B, p(res), p(loss), p(dy), None),
        (Ct.byref(ld), p(y), p(s), p(t), None, 0, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(ld), p(y), p(s), p(t), None, -5, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(bad_kind), p(y), p(s), p(t), None, B, p(res), p(loss), p(dy), p(ds)),
        (Ct.byref(ld), p(y) + 4, p(s), p(t), None, B - 1, p(res), p(loss), p(dy), p(ds)),
    ]
    for args in calls:
        assert lib.inr_gain_loss_grad(*args, st) == -1, args
        assert "inr_gain_loss_grad" in L.last_error()
    for args in ((None, p(s), B, p(res)), (p(y), None, B, p(res)), (p(y), p(s), B, None), (p(y), p(s), 0, p(res))):
        assert lib.inr_gain_apply(*args, st) == -1 and "inr_gain_apply" in L.last_error()
    torch.cuda.synchronize()
    for buf in (res, dy, ds, loss):
        assert bool((buf == sent).all())


# ---- the gain network's plan -------------------------------------------------------------------------------------------
def test_default_gain_network_against_float64(dev):
    """FFN 2 -> 512 x 8 -> 1 (the reference's, models/networks.py:388-394) at B = 300 through inr_forward / inr_backward:
    output and flat gradient at 1e-5 against float64"""
    import inr_mi355x as M
    from inr_mi355x.train_scaling import SCALER_NET
    torch.manual_seed(5)
    model = M.FFN(dict(SCALER_NET))
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in model.state_dict().items()}
    B = 300
    z = np.stack([rnd(B, 51, 1.0), np.abs(rnd(B, 52, 1.41))], axis=1)
    dout = rnd(B, 53, 1.0).reshape(B, 1)
    eng = model.to(dev)._engine()
    assert eng.in_features == 2 and eng.out_features == 1
    zd = to_dev(z)
    out = eng.forward(zd, None, save=True)
    grads = eng.backward(zd, None, to_dev(dout)).cpu().numpy()
    ref = O.ffn_forward(sd64, torch.from_numpy(z).double(), SCALER_NET)
    g64 = torch.autograd.grad((ref * torch.from_numpy(dout).double()).sum(), list(sd64.values()))
    e_out = rel_l2(out.cpu().numpy(), ref.detach().numpy())
    e_grad = rel_l2(grads, torch.cat([g.reshape(-1) for g in g64]).numpy())
    print("gain network 512 x 8: out", e_out, "grad", e_grad)
    from conftest import record_parity
    record_parity("gain:default_plan", out=e_out, grad=e_grad)
    assert out.shape == (B, 1) and e_out <= TOL and e_grad <= TOL, (e_out, e_grad)


# ---- the composite step ------------------------------------------------------------------------------------------------
SHAPE = (2, 16, 24)
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=64)
SNET = dict(network_input_size=2, network_output_size=1, network_depth=3, network_width=64)


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=200, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3), net=dict(NET),
               scaler=dict(network_width=64, network_depth=3))
    cfg.update(kw)
    return cfg


def _trainer(dev, undersampling):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_scaling import ScaledFitTrainer
    C_, H, W = SHAPE
    image = make_kspace(C_, H, W)[0]
    return ScaledFitTrainer(_cfg(undersampling=undersampling), image, grid_coords(C_, H, W, device=dev), SHAPE, dev, seed=3,
                            mask_seed=11)  # (the pattern is drawn per trainer: the same key gives every trainer the same mask)


class Ref64:
    """the composite in torch float64: gauss encoder, SIREN, FFN, res = y exp(-s), 0.5 MSE on the sampled rows, one
    stock torch.optim.Adam over both networks' parameters (train_scaling.py:69-70)"""

    def __init__(self, tr):
        d = lambda sd: {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
        self.b, self.s = d(tr.model.state_dict()), d(tr.scaler.state_dict())
        self.B = tr.encoder.B.cpu().double()
        cfg = tr.config
        self.opt = torch.optim.Adam(list(self.b.values()) + list(self.s.values()), lr=cfg["lr"],
                                    betas=(cfg["beta1"], cfg["beta2"]), weight_decay=cfg["weight_decay"])
        self.coords, self.z = tr.coords.cpu().double(), tr.z.cpu().double()
        self.gt = tr.image.cpu().double()
        self.mask = None if tr.mask_cpu is None else tr.mask_cpu.reshape(-1).bool()
        self.bs, self.n = tr.bs, tr.n

    @staticmethod
    def forward(b, s, B, coords, z):
        y = O.siren_forward(b, O.encode(coords, B, "gauss"), NET)
        return y * torch.exp(-O.ffn_forward(s, z, SNET))

    def step(self, it):
        lo, hi = it * self.bs, min((it + 1) * self.bs, self.n)
        res = self.forward(self.b, self.s, self.B, self.coords[lo:hi], self.z[lo:hi])
        sel = slice(None) if self.mask is None else self.mask[lo:hi]
        loss = O.loss_l2_half(res[sel], self.gt[lo:hi][sel])
        self.opt.zero_grad()
        loss.backward()
        flat = lambda sd: torch.cat([p.grad.reshape(-1) for p in sd.values()]).numpy().copy()
        out = float(loss.detach()), flat(self.b), flat(self.s)
        self.opt.step()
        return out


@pytest.fixture(scope="module", params=[None, "radial-4"], ids=["full", "radial4"])
def fit(dev, request):
    """(trainer after 3 steps, what was measured on the way): one fit per mask variant, shared by the tests below"""
    tr = _trainer(dev, request.param)
    assert tr.steps_per_epoch == 4 and tr._range(3) == (600, 768)  # the last batch is partial
    assert (tr.mask is None) == (request.param is None)
    ref = Ref64(tr)
    seen = {}
    for it in range(3):
        loss = float(tr.step(0, it))
        r_loss, r_gb, r_gs = ref.step(it)
        if it == 0:
            seen["step1"] = (loss, tr.engine.grads.cpu().numpy().copy(), tr.scaler_engine.grads.cpu().numpy().copy(),
                             r_loss, r_gb, r_gs)
    return tr, ref, seen


def test_first_step_against_float64_autograd(fit):
    """loss and the flat gradients of both engines after step 1 at 1e-5"""
    _, _, seen = fit
    loss, gb, gs, r_loss, r_gb, r_gs = seen["step1"]
    errs = dict(loss=abs(loss - r_loss) / abs(r_loss), backbone=rel_l2(gb, r_gb), scaler=rel_l2(gs, r_gs))
    print("step 1:", errs)
    assert np.linalg.norm(r_gs) > 0 and np.linalg.norm(r_gb) > 0
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_three_steps_against_float64_adam(fit):
    """the parameters of both networks after 3 steps, compared the way tests/test_gpu_configs.py::
    test_config1_siren_image_space compares a trainer's parameters with its reference's after two steps: relative L2 of
    the flat parameter vector, below 5e-5 -- here per engine, against stock float64 Adam.  That test says why the
    comparison is a norm and not entry by entry: Adam's first steps move an entry by about lr * sign(g), so an entry whose
    gradient is rounding noise may differ by a good part of a step.  One does here: entry (38, 31) of the backbone's
    model.1.linear.weight has a step-1 gradient of -6.5e-9, below Adam's eps = 1e-8, and ends 4.7e-6 from float64 on the
    MI355X -- and 4.3e-6 from it in a torch fp32 run of the same composite on the host, the only entry of either run
    beyond 2e-6."""
    tr, ref, _ = fit
    assert tr.engine.step == 3 and tr.scaler_engine.step == 3
    for name, eng, sd in (("backbone", tr.engine, ref.b), ("gain network", tr.scaler_engine, ref.s)):
        want = torch.cat([v.detach().reshape(-1) for v in sd.values()]).numpy()
        got = eng.params.cpu().numpy()
        e = rel_l2(got, want)
        print(f"params after 3 steps, {name}: rel L2 {e:.3e}, largest entry difference {np.abs(got - want).max():.3e}")
        assert got.shape == want.shape and e < 5e-5, (name, e)


def test_predict_all_against_float64_composite(fit):
    tr, ref, _ = fit
    d = lambda sd: {k: v.detach().cpu().double() for k, v in sd.items()}
    want = Ref64.forward(d(tr.model.state_dict()), d(tr.scaler.state_dict()), ref.B, ref.coords, ref.z)
    got = tr.predict_all(chunk=300)
    assert got.shape == (tr.n, 2)
    assert rel_l2(got.cpu().numpy(), want.numpy()) <= TOL
    g = tr.gain_summary
    s = O.ffn_forward(d(tr.scaler.state_dict()), ref.z, SNET).reshape(-1)
    gain = torch.exp(-s)
    assert g["width"] == 64 and g["depth"] == 3
    for k, v in (("min", gain.min()), ("max", gain.max()), ("mean", gain.mean())):
        assert abs(g[k] - float(v)) <= 1e-5 * float(v), (k, g[k], float(v))
    rec = tr.validate(0)
    assert rec["gain"] == tr.gain_summary and tr.val_history[-1]["gain"] == rec["gain"]
    assert rec["test_loss"] is not None and np.isfinite(rec["psnr"])
    assert tr.metrics()["gain"] == rec["gain"]


def test_resume_is_bit_identical(dev, fit):
    """save after 2 steps, load into a fresh trainer, one more step on each: parameters and Adam moments of both engines
    equal to the bit -- and to the uninterrupted fit's"""
    tr3, _, _ = fit
    und = tr3.config["undersampling"]
    a = _trainer(dev, und)
    a.fit(2)
    ckpt = a.checkpoint()
    assert [k.split(".")[0] for k in ckpt["net"]] == ["backbone"] * 6 + ["scaler"] * 6
    assert sorted(ckpt["opt"]["state"]) == list(range(12)) and ckpt["opt"]["param_groups"][0]["params"] == list(range(12))
    b = _trainer(dev, und)
    b.load_checkpoint(ckpt)
    assert b.engine.step == 2 and b.scaler_engine.step == 2
    a.step(0, 2)
    b.step(0, 2)
    for ea, eb, e3 in ((a.engine, b.engine, tr3.engine), (a.scaler_engine, b.scaler_engine, tr3.scaler_engine)):
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert _bits(getattr(ea, name), getattr(eb, name)), name
        assert _bits(ea.params, e3.params)
    from inr_mi355x.train import INRTrainer
    with pytest.raises(ValueError, match="train_scaling"):
        INRTrainer(_cfg(), a.image_full, a.coords, SHAPE, dev, seed=3).load_checkpoint(ckpt)


def test_reconstructor(dev, fit, tmp_path):
    """the native grid equals predict_all() bit for bit; --scale 2 equals the float64 composite on grid_rows_numpy's
    coordinates at 1e-5"""
    from inr_mi355x.grid import grid_rows_numpy
    from inr_mi355x.reconstruct import Reconstructor
    tr, ref, _ = fit
    path = str(tmp_path / "model.pt")
    torch.save(tr.checkpoint(), path)
    rec = Reconstructor(tr.config, path, shape=SHAPE, device=dev)
    assert rec.scaler is not None and rec.scaler_engine.exp_avg is None and rec.engine.exp_avg is None
    want = tr.predict_all(chunk=300)
    got = rec.render(chunk=300)
    assert got.shape == (*SHAPE, 2) and _bits(got.reshape(-1, 2), want), float((got.reshape(-1, 2) - want).abs().max())
    fine = rec.render(scale=2, chunk=1000)
    spec = rec.grid(scale=2)
    assert fine.shape == (2, 32, 48, 2)
    c, dist = grid_rows_numpy(spec, 0, spec.rows)
    d = lambda sd: {k: v.detach().cpu().double() for k, v in sd.items()}
    z = torch.from_numpy(np.stack([c[:, 0], dist], axis=1)).double()
    want64 = Ref64.forward(d(tr.model.state_dict()), d(tr.scaler.state_dict()), ref.B, torch.from_numpy(c).double(), z)
    assert rel_l2(fine.reshape(-1, 2).cpu().numpy(), want64.numpy()) <= TOL
    sub = rec.render(coils=[1], window=(-0.5, 0.25, 0.1, 0.7), height=5, width=7)
    assert sub.shape == (1, 5, 7, 2) and bool(torch.isfinite(sub).all())
