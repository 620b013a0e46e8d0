"""The tail of every training step (csrc/inr_params.hip) against the float64 / exact-tree references of
tests/step_tail_cases.py (``-m gpu``): every kernel path of the Adam update at edge entries, held to ``adam_bound`` of
``adam_ref64`` AND to the bits of the plain inr_adam_step path; the weight images after every update against a fresh
inr_pack_params; dead layers; the slab reduction against its own slabs, bit for bit.  Public entries only.

Each test prints its worst error / bound ratio (and records it through conftest.record_parity).

Left out: the loss word of a slab (its offset in a slab is not part of inr_plan_sizes: the conformance matrix holds
loss_out to the oracle), and the descriptor-walking fallback of adam_dead_ranges (more than 8 merged dead ranges: no plan
that inr_plan_create accepts has more than 6, tests/test_step_tail_host.py)."""
import os

import numpy as np
import pytest
import torch

import aux_bits_cases as A
import step_tail_cases as S
from aux_bits_cases import dev, rnd

pytestmark = pytest.mark.gpu

FULL = S.HYPER[-1]


def _lib():
    from inr_mi355x import _lib as L
    return L, L.load()


def _record(test, ratio, **kw):
    from conftest import record_parity
    print(f"{test}: worst error / adam_bound = {ratio:.3f}")
    record_parity("step_tail:" + test, ratio=ratio, **kw)


def _load(eng, state):
    for t, a in zip((eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq), state):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def _read(eng):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq))


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _plain(eng, state, step, betas, hyper):
    """inr_adam_step on ``state`` = fp32 (p, g, m, v): the path every other one is compared with"""
    L, lib = _lib()
    _load(eng, state)
    L.check(lib.inr_adam_step(eng.plan, eng.params.data_ptr(), eng.grads.data_ptr(), eng.exp_avg.data_ptr(),
                              eng.exp_avg_sq.data_ptr(), eng.packed.data_ptr(), S.LR, betas[0], betas[1], S.EPS, *hyper,
                              step, A._stream()))
    return _read(eng)


def _ratio(got, state, step, betas, hyper, live=None):
    args = (*state, step, S.LR, betas[0], betas[1], S.EPS, *hyper, live)
    return S.worst_ratio(got, S.adam_ref64(*args), S.adam_bound(*args))


def _images_current(eng):
    """eng.packed == what inr_pack_params writes from eng.params into a buffer of all-ones words (NaN as fp32 and as
    bf16), wherever that pack wrote; the plan gets its own buffer back afterwards"""
    L, lib = _lib()
    got = eng.packed.clone()
    fresh = torch.full((eng.packed_floats,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    L.check(lib.inr_pack_params(eng.plan, eng.params.data_ptr(), fresh.data_ptr(), A._stream()))
    L.check(lib.inr_pack_params(eng.plan, eng.params.data_ptr(), eng.packed.data_ptr(), A._stream()))
    torch.cuda.synchronize()
    word = torch.int16 if eng.desc.precision == L.PRECISION_BF16 else torch.int32  # bf16 plans: panels of 16-bit entries
    a, b = got.view(word).cpu().numpy(), fresh.view(word).cpu().numpy()
    wrote = b != -1
    assert int(wrote.sum()) >= eng.n_params  # (an entry lands in one image word at least, most in two or three)
    assert np.array_equal(a[wrote], b[wrote]), f"{int((a[wrote] != b[wrote]).sum())} image words are not the parameters'"


def _combos(complex_plan):
    hyper = S.HYPER_COMPLEX if complex_plan else S.HYPER
    return [(s, h, S.BETAS) for s in S.STEPS for h in hyper] + [(2, hyper[-1], S.BETAS_ONCE)]


def _edge_engine(plan):
    eng = A._engine(plan)
    tensors = S.tensors_of(plan)
    P = eng.n_params
    assert max(o + n for o, n in tensors) == P
    state = S.edge_state(P, tensors)
    eng.bind(dev(state[0]).clone())
    return eng, state


class _Env:
    """INR_PACK_BY_IMAGE set (or unset) and restored, as aux_bits_cases.step_case does"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("INR_PACK_BY_IMAGE")
        os.environ.pop("INR_PACK_BY_IMAGE", None)
        if self.value is not None:
            os.environ["INR_PACK_BY_IMAGE"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("INR_PACK_BY_IMAGE", None)
        if self.old is not None:
            os.environ["INR_PACK_BY_IMAGE"] = self.old


# ---- the update, path by path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["siren32", "wire", "wire2d", "gabor"])
def test_adam_pack_kernel(plan):
    """inr_adam_step (adam_pack_kernel): steps 1, 2, 1000, every penalty combination, both beta pairs; siren32's 2722
    entries end inside a workgroup and its workgroups span two or three layers (layer_walk)"""
    with _Env(None):
        eng, state = _edge_engine(plan)
        worst = 0.0
        for step, hyper, betas in _combos(plan in ("wire", "wire2d")):
            got = _plain(eng, state, step, betas, hyper)
            r = _ratio(got, state, step, betas, hyper)
            assert r <= 1.0, (plan, step, hyper, betas, r)
            worst = max(worst, r)
            _images_current(eng)
    _record(f"adam_pack/{plan}", worst)


def test_adam_by_image_path():
    """adam_shard_kernel + pack_images_real_kernel (INR_PACK_BY_IMAGE=1) on siren32"""
    with _Env(None):
        eng, state = _edge_engine("siren32")
    worst = 0.0
    for step, hyper, betas in _combos(False):
        with _Env(None):
            want = _plain(eng, state, step, betas, hyper)
        with _Env("1"):
            got = _plain(eng, state, step, betas, hyper)
            _images_current(eng)
        assert _same_bits(got, want), (step, hyper, betas)
        r = _ratio(got, state, step, betas, hyper)
        assert r <= 1.0, (step, hyper, betas, r)
        worst = max(worst, r)
    _record("by_image/siren32", worst)


def _shard(eng, bufs, g, lo, hi, step, betas, hyper):
    L, lib = _lib()
    L.check(lib.inr_adam_step_shard(eng.plan, bufs[0].data_ptr(), g[lo:].data_ptr() if lo < g.numel() else g.data_ptr(),
                                    bufs[1].data_ptr(), bufs[2].data_ptr(), lo, hi, S.LR, betas[0], betas[1], S.EPS, *hyper,
                                    step, A._stream()))


def test_adam_shard_partitions():
    """inr_adam_step_shard: the shards of a partition of [0, P), in any order, give the bits of the whole update, and a
    shard touches nothing outside [lo, hi) (NaN guards there, never read)"""
    with _Env(None):
        eng, state = _edge_engine("siren32")
        P = eng.n_params
        parts = {"one": [(0, P)], "three": [(0, 911), (911, 1817), (1817, P)], "reversed": [(1817, P), (911, 1817), (0, 911)],
                 "middle_first": [(911, 1817), (0, 911), (1817, P)], "empty": [(0, 1361), (1361, 1361), (1361, P)],
                 "empty_at_P": [(0, P), (P, P)]}
        g = dev(state[1])
        worst = 0.0
        for step, hyper, betas in ((1, FULL, S.BETAS), (2, FULL, S.BETAS), (1000, S.HYPER[1], S.BETAS), (2, FULL, S.BETAS_ONCE)):
            want = _plain(eng, state, step, betas, hyper)
            for name, shards in parts.items():
                bufs = [dev(state[k]) for k in (0, 2, 3)]
                for lo, hi in shards:
                    _shard(eng, bufs, g, lo, hi, step, betas, hyper)
                    guard = []
                    for k in (0, 2, 3):
                        a = np.full(P, np.nan, dtype=np.float32)
                        a[lo:hi] = state[k][lo:hi]
                        guard.append(dev(a))
                    before = [t.cpu().numpy().copy() for t in guard]
                    _shard(eng, guard, g, lo, hi, step, betas, hyper)
                    torch.cuda.synchronize()
                    for t, b, w in zip(guard, before, want):
                        a = t.cpu().numpy()
                        assert a[:lo].tobytes() == b[:lo].tobytes() and a[hi:].tobytes() == b[hi:].tobytes(), (name, lo, hi)
                        assert a[lo:hi].tobytes() == w[lo:hi].tobytes(), (name, lo, hi)
                torch.cuda.synchronize()
                got = tuple(t.cpu().numpy() for t in bufs)
                assert _same_bits(got, want), (name, step, hyper)
            r = _ratio(want, state, step, betas, hyper)
            assert r <= 1.0, (step, hyper, betas, r)
            worst = max(worst, r)
    _record("shard/siren32", worst)


def test_adam_step_dev_reads_the_clamped_entry():
    """inr_adam_step_dev with a 4-entry table: step_dev = 0, 3 inside it, 4 and 9 past its end -- the header says entry
    min(t, n_sched - 1), i.e. the update of step min(t, 3) + 1; step_dev ends at t + 1"""
    L, lib = _lib()
    with _Env(None):
        eng, state = _edge_engine("siren32")
        worst = 0.0
        for betas, hyper in ((S.BETAS, FULL), (S.BETAS, S.HYPER[0]), (S.BETAS_ONCE, FULL)):
            sched = np.empty(8, dtype=np.float32)
            L.check(lib.inr_adam_schedule(S.LR, betas[0], betas[1], 4, sched.ctypes.data))
            for k in range(4):  # the table is the fp32 of torch's doubles
                assert sched[2 * k] == np.float32(S.LR / (1.0 - betas[0] ** (k + 1)))
                assert sched[2 * k + 1] == np.float32(np.sqrt(1.0 - betas[1] ** (k + 1)))
            sched_dev = dev(sched)
            for t in (0, 3, 4, 9):
                step = min(t, 3) + 1
                want = _plain(eng, state, step, betas, hyper)
                _load(eng, state)
                step_dev = torch.full((1,), t, dtype=torch.int32, device="cuda")
                L.check(lib.inr_adam_step_dev(eng.plan, eng.params.data_ptr(), eng.grads.data_ptr(), eng.exp_avg.data_ptr(),
                                              eng.exp_avg_sq.data_ptr(), eng.packed.data_ptr(), sched_dev.data_ptr(), 4,
                                              step_dev.data_ptr(), betas[0], betas[1], S.EPS, *hyper, A._stream()))
                got = _read(eng)
                assert int(step_dev.item()) == t + 1
                assert _same_bits(got, want), (t, betas, hyper)
                r = _ratio(got, state, step, betas, hyper)
                assert r <= 1.0, (t, betas, hyper, r)
                worst = max(worst, r)
                _images_current(eng)
    _record("step_dev/siren32", worst)


def _step_inputs(eng, B):
    from inr_mi355x import _lib as L
    from inr_mi355x.engine import LossSpec
    x = dev(rnd(B * 3, 2).reshape(B, 3))
    enc_B = dev(rnd(eng.in_features // 2 * 3, 3, 2.0).reshape(-1, 3))
    gt = dev(rnd(B * 2, 4, 0.3).reshape(B, 2))
    return x, enc_B, gt, LossSpec(L.LOSS_L2_HALF, 1e-3, 2.0, 0.5, 3000)


def _reset(eng, p0, m0, v0, step):
    _load(eng, (p0, np.zeros_like(p0), m0, v0))
    eng.step = step - 1
    eng.pack()


def _fused_state(P):
    p0 = rnd(P, 1, 0.1)
    p0[0], p0[255], p0[256], p0[P - 1] = 0.0, -0.0, 0.0, -0.0
    return p0, rnd(P, 6, 1e-3), np.abs(rnd(P, 7, 1e-6))


@pytest.mark.parametrize("plan", ["siren32", "siren256"])
def test_reduce_adam_fused(plan):
    """inr_train_adam_step (reduce_adam_real_kernel): the gradient it leaves is that of inr_train_step bit for bit, and
    the update is adam_ref64 of that gradient within adam_bound -- and the plain path's bits"""
    with _Env(None):
        eng = A._engine(plan)
        P = eng.n_params
        B, _ = A._batch_for(eng, "3")
        p0, m0, v0 = _fused_state(P)
        eng.bind(dev(p0).clone())
        x, enc_B, gt, spec = _step_inputs(eng, B)
        worst = 0.0
        for step, hyper, betas, (m, v) in ((1, FULL, S.BETAS, (np.zeros_like(p0), np.zeros_like(p0))),
                                           (2, FULL, S.BETAS, (m0, v0)), (1000, S.HYPER[0], S.BETAS_ONCE, (m0, v0))):
            _reset(eng, p0, m, v, step)
            eng.train_step(x, enc_B, gt, spec)
            torch.cuda.synchronize()
            grads = eng.grads.cpu().numpy().copy()
            assert np.all(np.isfinite(grads)) and np.count_nonzero(grads) > P // 2
            state = (p0, grads, m, v)
            want = _plain(eng, state, step, betas, hyper)
            _reset(eng, p0, m, v, step)
            eng.train_adam_step(x, enc_B, gt, spec, S.LR, beta1=betas[0], beta2=betas[1], eps=S.EPS, weight_decay=hyper[0],
                                l1=hyper[1], l2=hyper[2])
            got = _read(eng)
            assert eng.grads.cpu().numpy().tobytes() == grads.tobytes()
            assert _same_bits(got, want), (step, hyper, betas)
            r = _ratio(got, state, step, betas, hyper)
            assert r <= 1.0, (step, hyper, betas, r)
            worst = max(worst, r)
            _images_current(eng)
    _record(f"reduce_adam/{plan}", worst)


def test_images_after_update_bf16():
    """siren256_bf16: the panel images and the bias table after inr_adam_step and after inr_train_adam_step are those of
    a fresh pack of the updated parameters; the update itself is fp32 and held to adam_bound"""
    with _Env(None):
        eng = A._engine("siren256_bf16")
        P = eng.n_params
        B, _ = A._batch_for(eng, "3")
        p0, m0, v0 = _fused_state(P)
        eng.bind(dev(p0).clone())
        x, enc_B, gt, spec = _step_inputs(eng, B)
        state = (p0, rnd(P, 5, 1e-2), m0, v0)
        got = _plain(eng, state, 2, S.BETAS, FULL)
        worst = _ratio(got, state, 2, S.BETAS, FULL)
        _images_current(eng)
        _reset(eng, p0, m0, v0, 2)
        eng.train_adam_step(x, enc_B, gt, spec, S.LR, eps=S.EPS, weight_decay=FULL[0], l1=FULL[1], l2=FULL[2])
        got = _read(eng)
        grads = eng.grads.cpu().numpy().copy()
        assert np.all(np.isfinite(grads))
        worst = max(worst, _ratio(got, (p0, grads, m0, v0), 2, S.BETAS, FULL))
        _images_current(eng)
    assert worst <= 1.0
    _record("bf16_images/siren256_bf16", worst)


@pytest.mark.parametrize("depth", [2, 8])
def test_dead_layers_keep_their_bits(depth):
    """MultiscaleKFourier with unused heads and stages (3 merged dead ranges at depth 2, 6 at depth 8; both the range
    form of adam_dead_ranges): under weight decay and a gradient that is nonzero there, dead parameters keep their bits
    and their moments stay exactly 0 -- through inr_adam_step and through inr_adam_step_shard"""
    with _Env(None):
        eng, tensors, live = S.multiscale(depth)
        P = eng.n_params
        assert len(S.dead_ranges(tensors, live)) == (3 if depth == 2 else 6)
        p, g, m, v = S.edge_state(P, tensors)
        m[~live] = 0.0
        v[~live] = 0.0
        state = (p, g, m, v)
        assert np.count_nonzero(g[~live]) > 0.9 * (~live).sum() and np.count_nonzero(p[~live]) > 0.9 * (~live).sum()
        eng.bind(dev(p).clone())
        worst = 0.0
        for step, hyper in ((1, FULL), (2, S.HYPER[1]), (1000, FULL)):
            got = _plain(eng, state, step, S.BETAS, hyper)
            _images_current(eng)
            bufs = [dev(state[k]) for k in (0, 2, 3)]
            for lo, hi in ((0, P // 3 + 1), (P // 3 + 1, P)):
                _shard(eng, bufs, dev(g), lo, hi, step, S.BETAS, hyper)
            torch.cuda.synchronize()
            sharded = tuple(t.cpu().numpy() for t in bufs)
            for res in (got, sharded):
                assert res[0][~live].tobytes() == p[~live].tobytes()
                assert not res[1][~live].any() and not res[2][~live].any()
                assert not np.signbit(res[1][~live]).any() and not np.signbit(res[2][~live]).any()
                r = _ratio(res, state, step, S.BETAS, hyper, live)
                assert r <= 1.0, (depth, step, hyper, r)
                worst = max(worst, r)
            assert _same_bits(sharded, got)
    _record(f"dead_layers/depth{depth}", worst)


# ---- the slab reduction against its own slabs -----------------------------------------------------------------------
@pytest.mark.parametrize("target", S.SLAB_COUNTS)
def test_flat_slab_sum_is_its_tree(target):
    """siren32 (flat slab layout, no GEMM chunk slabs): after a step the workspace still holds the slabs; the gradient is
    flat_sum_ref32 of them bit for bit, within the textbook bound of their float64 sum, and the same on a second call --
    from reduce_slabs_real_kernel (inr_train_step) and from reduce_adam_real_kernel (inr_train_adam_step)"""
    with _Env(None):
        eng = A._engine("siren32")
        P, sf = eng.n_params, eng.slab_floats
        B, nb = A._batch_for(eng, target)
        assert eng.workspace(B)[1] == eng.launch_dims(B)[1] == nb and (target == "33+" or nb == int(target))
        p0 = rnd(P, 1, 0.1)
        eng.bind(dev(p0).clone())
        x, enc_B, gt, spec = _step_inputs(eng, B)

        def slabs_and_grads():
            torch.cuda.synchronize()
            assert eng._slabs.numel() >= nb * sf
            slabs = eng._slabs[:nb * sf].view(nb, sf)[:, :P].cpu().numpy().copy()
            return slabs, eng.grads.cpu().numpy().copy()

        eng.train_step(x, enc_B, gt, spec)
        slabs, grads = slabs_and_grads()
        assert np.all(np.isfinite(slabs)) and np.count_nonzero(slabs.sum(axis=0)) > P // 2
        assert grads.tobytes() == S.flat_sum_ref32(slabs).tobytes()
        s64, bound = S.flat_sum_ref64(slabs)
        err = np.abs(grads.astype(np.float64) - s64)
        assert np.all(err <= bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.where(err == 0, 0.0, err / bound).max())
        eng.grads.zero_()
        eng.train_step(x, enc_B, gt, spec)
        slabs2, grads2 = slabs_and_grads()
        assert slabs2.tobytes() == slabs.tobytes() and grads2.tobytes() == grads.tobytes()
        eng.grads.zero_()
        eng.train_adam_step(x, enc_B, gt, spec, S.LR, weight_decay=1e-4)
        slabs3, grads3 = slabs_and_grads()
        assert slabs3.tobytes() == slabs.tobytes() and grads3.tobytes() == grads.tobytes()
    from conftest import record_parity
    print(f"flat_slab_sum/{nb} slabs: worst error / textbook bound = {ratio:.3f}")
    record_parity(f"step_tail:flat_slab_sum/{target}", slabs=nb, ratio=ratio)
