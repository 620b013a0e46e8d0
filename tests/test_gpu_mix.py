"""Mixture of heads on the MI355X (``-m gpu``): inr_mix_loss_grad / inr_mix_apply against the float64
statement of inr_mi355x/mix.py and the float32 statement of ``res``, and MixtureFitTrainer / Reconstructor against torch
float64 autograd of the composite written out here.

Criteria -- none of them new: 1e-5 relative L2 per array and 1e-5 relative on the loss words against float64 (the
criterion of tests/test_gpu_gain.py); parameters after three steps as that file compares them (relative L2 of the flat
vector below 5e-5, per engine); bit equality wherever the same kernels see the same inputs, and of ``res`` with
mix_numpy_f32.  Rows whose float64 |pre_c| lies within 1e-6 of 1 may fall on the other side of the clamp in fp32: they are
left out of the dy / dw comparison and must be at most 1 % of the rows (tests/test_mix_host.py: with these inputs there are
none)."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import loss_cases as C
import mix_cases as MC
import oracle as O  # checker only
from aux_bits_cases import _stream, dev as to_dev, rnd

pytestmark = pytest.mark.gpu

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


def _rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _call(kind, ys, w, gt, dist, radii, inv, m, detach, clamp, want_res=True):
    from inr_mi355x import mix as M
    out, res, dys, dw = M.mix_loss_grad(_spec(kind), ys, w, gt, dist, radii, inv, mask=m, detach=detach, clamp=clamp,
                                        hdr_A=C.HDR_A, want_res=want_res)
    torch.cuda.synchronize()
    return out[:len(ys) + 2].clone(), res, dys, dw


# ---- the kernel against the float64 statement --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(C.KINDS))
def test_kernel_against_float64(dev, kind):
    """every size x K x mask x detach x clamp, both amplitude sets: the total, each of the K + 1 terms, every dy_k and dw
    at 1e-5; res equal to mix_numpy_f32 bit for bit; unsampled rows exactly 0; an all-zero mask gives 0 throughout; res =
    NULL and a second call give the same bits; inr_mix_apply equals res bit for bit, in place too"""
    from inr_mi355x import mix as M
    worst = {}
    for B in MC.SIZES:
        for K in MC.HEADS:
            for amp in MC.AMPS:
                ys, w, gt, dist, radii = MC.rows(kind, B, K, amp)
                yd, wd, td, dd = [to_dev(y) for y in ys], to_dev(w), to_dev(gt), to_dev(dist)
                for clamp in (True, False):
                    res32 = M.mix_numpy_f32(ys, w, clamp)[1]
                    for tag in MC.MASKS:
                        m = MC.mask_of(tag, B)
                        md = None if m is None else to_dev(m)
                        inv = M.inv_counts(M.ring_counts(dist, m, radii))
                        for detach in (True, False):
                            what = (kind, B, K, amp, clamp, tag, detach)
                            ref = M.mix_loss_grad_numpy(_spec(kind), ys, w, gt, dist, m, radii, detach=detach,
                                                        clamp=clamp, hdr_A=C.HDR_A)
                            words, res, dys, dw = _call(kind, yd, wd, td, dd, radii, inv, md, detach, clamp)
                            words_h = words.cpu().numpy().astype(np.float64)
                            res_h, dw_h = res.cpu().numpy(), dw.cpu().numpy()
                            dys_h = [d.cpu().numpy() for d in dys]
                            assert all(np.all(np.isfinite(a)) for a in [words_h, res_h, dw_h] + dys_h), what
                            assert np.array_equal(res_h.view(np.int32), res32.view(np.int32)), what + ("res bits",)
                            near = MC.near_clamp(ref[2]) if clamp else np.zeros(B, dtype=bool)
                            assert near.sum() <= MC.NEAR_CAP * B, what + ("near the clamp", int(near.sum()))
                            keep = ~near
                            errs = dict(loss=_rel(words_h[0], ref[0]), dw=rel_l2(dw_h[keep], ref[5][keep]))
                            for t in range(K + 1):
                                errs[f"term{t}"] = _rel(words_h[1 + t], ref[1][t])
                            for k in range(K):
                                errs[f"dy{k}"] = rel_l2(dys_h[k][keep], ref[4][k][keep])
                            for name, v in errs.items():
                                key = name.rstrip("0123456789")
                                worst[key] = max(worst.get(key, 0.0), v)
                                assert v <= TOL, what + (name, v)
                            if m is not None:
                                assert not dw_h[m == 0].any() and not any(d[m == 0].any() for d in dys_h), what
                            if tag == "zeros":
                                assert not words_h.any() and not dw_h.any() and not any(d.any() for d in dys_h), what
                            if detach and clamp:  # the same kernel whatever the flags: once per mask is enough
                                w2, none, dys2, dw2 = _call(kind, yd, wd, td, dd, radii, inv, md, detach, clamp, False)
                                assert none is None and _bits(w2, words) and _bits(dw2, dw), what + ("res = NULL",)
                                assert all(_bits(a, b) for a, b in zip(dys2, dys)), what + ("res = NULL",)
                                w3, res3, dys3, dw3 = _call(kind, yd, wd, td, dd, radii, inv, md, detach, clamp)
                                assert _bits(w3, words) and _bits(res3, res) and _bits(dw3, dw), what + ("twice",)
                                assert all(_bits(a, b) for a, b in zip(dys3, dys)), what + ("twice",)
                    applied = M.mix_apply(yd, wd, clamp=clamp)
                    assert np.array_equal(applied.cpu().numpy().view(np.int32), res32.view(np.int32))
                    first = yd[0].clone()
                    assert M.mix_apply([first] + yd[1:], wd, clamp=clamp, out=first) is first and _bits(first, applied)
    print(kind, {k: f"{v:.2e}" for k, v in worst.items()})
    from conftest import record_parity
    record_parity("mix:kernel/" + kind, **worst)


@pytest.mark.parametrize("K", (3, 4))
def test_alignment_changes_no_bit(dev, K):
    """views that start one row into a buffer (8-byte aligned y_k / gt, 4K-byte aligned w, 4-byte aligned dist): the
    narrow accesses give the bits of the wide ones"""
    from inr_mi355x import mix as M
    B = 777
    ys, w, gt, dist, radii = MC.rows("hdr", B + 1, K, 1.0)
    m = MC.mask_of("random", B + 1)
    yd, wd, td, dd, md = [to_dev(y) for y in ys], to_dev(w), to_dev(gt), to_dev(dist), to_dev(m)
    inv = M.inv_counts(M.ring_counts(dist[1:], m[1:], radii))
    cut = lambda t: t[1:]
    a = _call("hdr", [cut(y).clone() for y in yd], cut(wd).clone(), cut(td).clone(), cut(dd).clone(), radii, inv,
              cut(md).clone(), False, True)
    assert cut(yd[0]).data_ptr() % 16 == 8 and cut(dd).data_ptr() % 8 == 4
    b = _call("hdr", [cut(y) for y in yd], cut(wd), cut(td), cut(dd), radii, inv, cut(md), False, True)
    assert _bits(a[0], b[0]) and _bits(a[1], b[1]) and _bits(a[3], b[3])
    assert all(_bits(p, q) for p, q in zip(a[2], b[2]))
    assert _bits(M.mix_apply([cut(y) for y in yd], cut(wd)), a[1])


def test_bad_arguments_leave_the_outputs_alone(dev):
    from inr_mi355x import _lib as L
    lib = L.load()
    B, K = 64, 3
    ys, w, gt, dist, radii = MC.rows("l2", B, K, 0.3)
    ys, w, gt, dist = [to_dev(y) for y in ys], to_dev(w), to_dev(gt), to_dev(dist)
    sent = 123.25
    res, dw = torch.full((B, 2), sent, device=dev), torch.full((B, K), sent, device=dev)
    dys = [torch.full((B, 2), sent, device=dev) for _ in range(K)]
    loss = torch.full((L.LOSS_WORDS,), sent, device=dev)
    ld = L.LossDesc(kind=0, eps=1e-3, sigma=2.0, factor=0.5, inv_count=1.0 / B, hdr_A=0.0)
    p = lambda x: x.data_ptr()

    def desc(n_heads=K, radii=radii, y_null=None, dy_null=None, y_off=0):
        d = L.MixDesc(n_heads=n_heads, detach=1, clamp=1)
        for k in range(K):
            d.y[k] = None if k == y_null else p(ys[k]) + y_off
            d.dy[k] = None if k == dy_null else p(dys[k])
        for k, r in enumerate(radii):
            d.radii[k] = r
        for k in range(K + 1):
            d.inv_count[k] = 1.0 / B
        return d

    good = desc()
    st = _stream()
    full = lambda d=good, ldp=ld, **kw: dict(dict(loss=Ct.byref(ldp) if ldp is not None else None,
                                                  mix=Ct.byref(d) if d is not None else None, w=p(w), gt=p(gt), dist=p(dist),
                                                  mask=None, B=B, res=p(res), loss_out=p(loss), dw=p(dw)), **kw)
    calls = [full(ldp=None), full(d=None), full(w=None), full(gt=None), full(dist=None), full(loss_out=None), full(dw=None),
             full(B=0), full(B=-5), full(d=desc(n_heads=1)), full(d=desc(n_heads=9)), full(d=desc(n_heads=0)),
             full(d=desc(y_null=K - 1)), full(d=desc(dy_null=0)),
             full(d=desc(radii=[0.0, 0.4, 0.4, 1.2])), full(d=desc(radii=[0.0, 0.8, 0.4, 1.2])),
             full(d=desc(radii=[0.0, float("nan"), 0.8, 1.2])),
             full(ldp=L.LossDesc(kind=7, inv_count=1.0)), full(ldp=L.LossDesc(kind=-1, inv_count=1.0)),
             full(d=desc(y_off=4), B=B - 1), full(gt=p(gt) + 4, B=B - 1)]
    for kw in calls:
        assert lib.inr_mix_loss_grad(*kw.values(), st) == -1, kw
        assert "inr_mix_loss_grad" in L.last_error()
    for args in ((None, p(w), B, p(res)), (Ct.byref(good), None, B, p(res)), (Ct.byref(good), p(w), B, None),
                 (Ct.byref(good), p(w), 0, p(res)), (Ct.byref(desc(n_heads=9)), p(w), B, p(res)),
                 (Ct.byref(desc(y_null=1)), p(w), B, p(res))):
        assert lib.inr_mix_apply(*args, st) == -1 and "inr_mix_apply" in L.last_error()
    assert lib.inr_mix_loss_grad(*full().values(), st) == 0  # the good descriptor itself is accepted ...
    torch.cuda.synchronize()
    assert not bool((dw == sent).any())
    res.fill_(sent), dw.fill_(sent), loss.fill_(sent)
    [d.fill_(sent) for d in dys]
    for kw in calls:  # ... and after it the refused calls still write nothing
        assert lib.inr_mix_loss_grad(*kw.values(), st) == -1
    torch.cuda.synchronize()
    for buf in [res, dw, loss] + dys:
        assert bool((buf == sent).all())


# ---- the composite step ------------------------------------------------------------------------------------------------
SHAPE = (3, 16, 12)
NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32)
GNET = dict(network_input_size=2, network_output_size=3, network_depth=3, network_width=16)
RADII = (0.0, 0.55, 0.95, 1.5)
FITS = [(None, True), ("radial-4", False)]
# The seed of the initial weights.  Three Adam steps are compared in fp32 against float64, and Adam's first steps move an
# entry by about lr sign(g): where a step-1 gradient lies below Adam's eps = 1e-8 the comparison measures fp32 itself, not
# the kernels (tests/test_gpu_gain.py::test_three_steps_against_float64_adam).  Width-32 experts trained on one ring
# often start with a hidden unit whose gradient is that small: a torch fp32 run of this file's Ref64 ON THE HOST, against
# its own float64 run, ends at a relative L2 of 2.4e-4 (detach) / 1.1e-5 (joint) with seed 3 (146 entries of expert 1
# beyond 2e-6, step-1 gradient 3e-9 at the worst), and beyond 5e-5 in one of the two with seeds 0, 4 and 5 as well.  With
# seed 1 the host fp32 run ends at 4.9e-7 / 3.0e-7 (seeds 2 and 6: below 1e-6 too).  The seed was picked by that host
# comparison alone.
SEED = 1


def _cfg(**kw):
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=97, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3), net=dict(NET),
               mixture=dict(gate=dict(network_width=16, network_depth=3)))
    cfg.update(kw)
    return cfg


def _trainer(dev, undersampling, detach):
    from inr_mi355x.grid import grid_coords
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_multihead import MixtureFitTrainer
    C_, H, W = SHAPE
    image = make_kspace(C_, H, W)[0]
    cfg = _cfg(undersampling=undersampling)
    cfg["mixture"]["detach"] = detach
    return MixtureFitTrainer(cfg, image, grid_coords(C_, H, W, device=dev), SHAPE, dev, seed=SEED, mask_seed=11,
                             radii=RADII)


class Ref64:
    """the composite in torch float64: gauss encoder, K SIRENs, the FFN gate on z, res = clamp(sum_k w_k y_k, -1, 1) with
    the experts detached in the mix when ``detach``, 0.5 MSE on the sampled rows plus each expert's 0.5 MSE on the sampled
    rows of its ring (both ends included), one stock torch.optim.Adam over experts then gate"""

    def __init__(self, tr):
        d = lambda sd: {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
        self.e, self.g = [d(m.state_dict()) for m in tr.models], d(tr.gate.state_dict())
        self.B = tr.encoder.B.cpu().double()
        cfg = tr.config
        params = [p for sd in self.e for p in sd.values()] + list(self.g.values())
        self.opt = torch.optim.Adam(params, lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]),
                                    weight_decay=cfg["weight_decay"])
        self.coords, self.z = tr.coords.cpu().double(), tr.z.cpu().double()
        self.dist32 = tr.dist.cpu()
        self.gt = tr.image.cpu().double()
        self.mask = None if tr.mask_cpu is None else tr.mask_cpu.reshape(-1).bool()
        self.bs, self.n, self.radii, self.detach = tr.bs, tr.n, tr.radii, tr.mixture["detach"]

    @staticmethod
    def forward(e, g, B, coords, z, detach=False):
        x = O.encode(coords, B, "gauss")
        ys = [O.siren_forward(sd, x, NET) for sd in e]
        w = O.ffn_forward(g, z, GNET)
        pre = sum(w[:, k:k + 1] * (y.detach() if detach else y) for k, y in enumerate(ys))
        return torch.clamp(pre, -1.0, 1.0), ys, w

    def step(self, it):
        lo, hi = it * self.bs, min((it + 1) * self.bs, self.n)
        res, ys, _ = self.forward(self.e, self.g, self.B, self.coords[lo:hi], self.z[lo:hi], self.detach)
        live = torch.ones(hi - lo, dtype=torch.bool) if self.mask is None else self.mask[lo:hi]
        gt = self.gt[lo:hi]
        terms = [O.loss_l2_half(res[live], gt[live])]
        d = self.dist32[lo:hi]
        for k, y in enumerate(ys):
            sel = live & (d >= self.radii[k]) & (d <= self.radii[k + 1])
            terms.append(O.loss_l2_half(y[sel], gt[sel]) if bool(sel.any()) else y.sum() * 0.0)
        loss = sum(terms)
        self.opt.zero_grad()
        loss.backward()
        flat = lambda sd: torch.cat([p.grad.reshape(-1) for p in sd.values()]).numpy().copy()
        out = float(loss.detach()), [float(t.detach()) for t in terms], [flat(sd) for sd in self.e], flat(self.g)
        self.opt.step()
        return out


@pytest.fixture(scope="module", params=FITS, ids=["full-detach", "radial4-joint"])
def fit(dev, request):
    """(trainer after 3 steps, its float64 twin, what was measured on the way): one fit per variant, shared below"""
    und, detach = request.param
    tr = _trainer(dev, und, detach)
    assert tr.steps_per_epoch == 6 and tr._range(5) == (485, 576) and tr.K == 3  # the last batch is partial
    assert (tr.mask is None) == (und is None)
    ref = Ref64(tr)
    seen = {}
    for it in range(3):
        loss = float(tr.step(0, it))
        r = ref.step(it)
        if it == 0:
            seen["step1"] = (loss, tr.loss_terms(), [e.grads.cpu().numpy().copy() for e in tr.engines],
                             tr.gate_engine.grads.cpu().numpy().copy()) + r
    return tr, ref, seen


def test_first_step_against_float64_autograd(fit):
    """the loss, its K + 1 terms and the flat gradients of all K + 1 engines after step 1 at 1e-5"""
    _, _, seen = fit
    loss, terms, ge, gg, r_loss, r_terms, r_ge, r_gg = seen["step1"]
    errs = dict(loss=_rel(loss, r_loss), gate=rel_l2(gg, r_gg))
    for t, (a, b) in enumerate(zip(terms, r_terms)):
        errs[f"term{t}"] = _rel(a, b)
    for k, (a, b) in enumerate(zip(ge, r_ge)):
        errs[f"expert{k}"] = rel_l2(a, b)
        assert np.linalg.norm(b) > 0
    print("step 1:", errs)
    from conftest import record_parity
    record_parity("mix:step1", **errs)
    assert len(terms) == 4 and np.linalg.norm(r_gg) > 0
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_three_steps_against_float64_adam(fit):
    """the parameters of every network after 3 steps, compared as tests/test_gpu_gain.py compares them: relative L2 of the
    flat parameter vector below 5e-5, per engine, against stock float64 Adam"""
    tr, ref, _ = fit
    pairs = [(f"expert {k}", e, sd) for k, (e, sd) in enumerate(zip(tr.engines, ref.e))] + [("gate", tr.gate_engine, ref.g)]
    for name, eng, sd in pairs:
        assert eng.step == 3
        want = torch.cat([v.detach().reshape(-1) for v in sd.values()]).numpy()
        got = eng.params.cpu().numpy()
        e = rel_l2(got, want)
        print(f"params after 3 steps, {name}: rel L2 {e:.3e}, largest entry difference {np.abs(got - want).max():.3e}")
        assert got.shape == want.shape and e < 5e-5, (name, e)


def test_predict_all_against_float64_composite(fit):
    tr, ref, _ = fit
    d = lambda sd: {k: v.detach().cpu().double() for k, v in sd.items()}
    want, _, w = Ref64.forward([d(m.state_dict()) for m in tr.models], d(tr.gate.state_dict()), ref.B, ref.coords, ref.z)
    got = tr.predict_all(chunk=300)
    assert got.shape == (tr.n, 2)
    assert rel_l2(got.cpu().numpy(), want.numpy()) <= TOL
    s = tr.mixture_summary
    assert s["heads"] == 3 and s["detach"] == tr.mixture["detach"] and s["clamp"] is True and s["radii"] == tr.radii
    assert s["gate_width"] == 16 and s["gate_depth"] == 3
    for k in range(3):
        for name, v in (("min", w[:, k].min()), ("max", w[:, k].max()), ("mean", w[:, k].mean())):
            assert abs(s["gate"][name][k] - float(v)) <= 1e-5 * float(v), (name, k)
    rec = tr.validate(0)
    assert rec["mixture"] == tr.mixture_summary and tr.val_history[-1]["mixture"] == rec["mixture"]
    assert len(rec["mixture"]["gate"]["mean"]) == 3 and len(rec["loss_terms"]) == 4
    assert rec["loss_terms"] == tr.loss_terms()
    assert rec["test_loss"] is not None and np.isfinite(rec["psnr"])
    assert tr.metrics()["mixture"] == rec["mixture"]


def test_resume_is_bit_identical(dev, fit):
    """save after 2 steps, load into a fresh trainer, one more step on each: parameters and Adam moments of all engines
    equal to the bit -- and to the uninterrupted fit's; other fits' checkpoints are refused by name"""
    tr3, _, _ = fit
    und, detach = tr3.config["undersampling"], tr3.mixture["detach"]
    a = _trainer(dev, und, detach)
    a.fit(2)
    ckpt = a.checkpoint()
    assert [k.split(".")[0] for k in ckpt["net"]] == ["heads"] * 18 + ["weighted_avg"] * 6
    assert list(ckpt["net"])[6].startswith("heads.1.") and "weighted_avg.model.0.weight" in ckpt["net"]
    assert sorted(ckpt["opt"]["state"]) == list(range(24)) and ckpt["opt"]["param_groups"][0]["params"] == list(range(24))
    assert ckpt["mixture"] == dict(radii=a.radii, detach=detach, clamp=True)
    b = _trainer(dev, und, detach)
    b.load_checkpoint(ckpt)
    assert all(e.step == 2 for e in b.engines + [b.gate_engine])
    a.step(0, 2)
    b.step(0, 2)
    for ea, eb, e3 in zip(a.engines + [a.gate_engine], b.engines + [b.gate_engine], tr3.engines + [tr3.gate_engine]):
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert _bits(getattr(ea, name), getattr(eb, name)), name
        assert _bits(ea.params, e3.params)
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_scaling import ScaledFitTrainer
    plain = INRTrainer(_cfg(), a.image_full, a.coords, SHAPE, dev, seed=3).checkpoint()
    with pytest.raises(ValueError, match=r"inr_mi355x\.train\)"):
        b.load_checkpoint(plain)
    scaled = ScaledFitTrainer(_cfg(scaler=dict(network_width=16, network_depth=3)), a.image_full, a.coords, SHAPE, dev,
                              seed=3).checkpoint()
    with pytest.raises(ValueError, match="train_scaling"):
        b.load_checkpoint(scaled)


def test_reconstructor(dev, fit, tmp_path):
    """the native grid equals predict_all() bit for bit; --scale 2 equals the float64 composite on grid_rows_numpy's
    coordinates at 1e-5"""
    from inr_mi355x.grid import grid_rows_numpy
    from inr_mi355x.reconstruct import Reconstructor
    tr, ref, _ = fit
    path = str(tmp_path / "model.pt")
    torch.save(tr.checkpoint(), path)
    rec = Reconstructor(tr.config, path, shape=SHAPE, device=dev)
    assert len(rec.experts) == 3 and rec.gate_engine.exp_avg is None and all(e.exp_avg is None for e in rec.expert_engines)
    want = tr.predict_all(chunk=300)
    got = rec.render(chunk=300)
    assert got.shape == (*SHAPE, 2) and _bits(got.reshape(-1, 2), want), float((got.reshape(-1, 2) - want).abs().max())
    fine = rec.render(scale=2, chunk=1000)
    spec = rec.grid(scale=2)
    assert fine.shape == (3, 32, 24, 2)
    c, dist = grid_rows_numpy(spec, 0, spec.rows)
    d = lambda sd: {k: v.detach().cpu().double() for k, v in sd.items()}
    z = torch.from_numpy(np.stack([c[:, 0], dist], axis=1)).double()
    want64 = Ref64.forward([d(m.state_dict()) for m in tr.models], d(tr.gate.state_dict()), ref.B,
                           torch.from_numpy(c).double(), z)[0]
    assert rel_l2(fine.reshape(-1, 2).cpu().numpy(), want64.numpy()) <= TOL
