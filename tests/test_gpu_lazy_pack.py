"""Weight images on demand on the GPU (``-m gpu``): a row-split plan's fused Adam step rewrites only the image family its
own kernel read, and whoever reads a stale family re-packs it first.  Everything here is held BITWISE to the eager
library (INR_LAZY_PACK=0, same process; laziness is opt-in: INR_LAZY_PACK=1): losses, parameters, moments, outputs -- and the lazily kept ``packed`` buffer to a
full pack of the same parameters, set by set as the readers validate them."""
import contextlib
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

E = 32  # encoder size: in_features 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make(dev, width, depth, seed=0):
    """(model, encoder, fused engine over the model's flat parameters)"""
    import inr_mi355x as M
    torch.manual_seed(seed)
    enc = M.Positional_Encoder(dict(embedding="gauss", scale=2, embedding_size=E, coordinates_size=3), device=dev)
    model = M.SIREN(dict(network_input_size=2 * E, network_output_size=2, network_depth=depth, network_width=width)).to(dev)
    return model, enc, model.fused_engine(E)


def data(dev, B, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, 3, generator=g) * 2 - 1).to(dev)
    gt = (torch.randn(B, 2, generator=g) * 0.3).to(dev)
    return x, gt


def spec():
    from inr_mi355x import _lib as L
    from inr_mi355x.engine import LossSpec
    return LossSpec(L.LOSS_L2_HALF, 1e-3, 2.0, 0.5, 3000)


def state(eng):
    valid, lazy = C.c_int32(-1), C.c_int32(-1)
    from inr_mi355x import _lib as L
    L.check(eng.lib.inr_plan_image_sets(eng.plan, C.byref(valid), C.byref(lazy)))
    return valid.value, lazy.value


def step(eng, enc, x, gt, rs):
    with env(INR_RS=rs):
        return float(eng.train_adam_step(x, enc.B, gt, spec(), 1e-3, weight_decay=1e-4))


def switching_run(dev, width, depth, B, lazy):
    """6 steps that alternate the two fused kernels, then inr_forward on 200 rows"""
    from inr_mi355x import _lib as L
    with env(INR_LAZY_PACK=lazy, INR_RS=None):
        model, enc, eng = make(dev, width, depth)
        # the remapped update's edge: P is no multiple of the lane's 4 entries or of the workgroup's 256
        assert eng.n_params % 4 != 0 and eng.n_params % 256 != 0, eng.n_params
        info = L.StepInfo()
        with env(INR_RS="1"):
            L.check(eng.lib.inr_plan_step_info(eng.plan, B, C.byref(info)))
        assert info.row_split == 1  # the plan has both kernels: there is something to be lazy about
        x, gt = data(dev, B)
        losses, seen = [], []
        for s in range(6):
            losses.append(step(eng, enc, x, gt, "1" if s % 2 == 0 else "0"))
            seen.append(state(eng)[0])
        x2, _ = data(dev, 200, seed=2)
        out = eng.forward(x2, enc.B).clone()
        seen.append(state(eng)[0])
        torch.cuda.synchronize()
        return dict(losses=losses, seen=seen, params=eng.params.clone(), m1=eng.exp_avg.clone(), m2=eng.exp_avg_sq.clone(),
                    grads=eng.grads.clone(), out=out)


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@pytest.mark.parametrize("width,depth,B", [(256, 3, 127), (256, 3, 1000), (256, 5, 1000), (160, 3, 127), (160, 3, 1000)])
def test_kernel_switches_match_eager(dev, width, depth, B):
    """width 160: K = 160 is no power of two (the division path of the image index); depth 5: the graded depth."""
    from inr_mi355x import _lib as L
    lazy, eager = switching_run(dev, width, depth, B, "1"), switching_run(dev, width, depth, B, "0")
    rs, mlp = L.IMG_RS, L.IMG_FWD | L.IMG_TR
    assert lazy["seen"] == [rs, mlp, rs, mlp, rs, mlp, mlp]  # every step found its family stale and left only it valid
    assert eager["seen"] == [L.IMG_ALL] * 7
    assert [x.hex() for x in lazy["losses"]] == [x.hex() for x in eager["losses"]]
    for k in ("params", "m1", "m2", "grads", "out"):
        same_bits(lazy[k], eager[k], k)
    assert all(l == l and abs(l) < 1e6 for l in lazy["losses"]) and float(lazy["out"].abs().max()) > 0


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("B", [127, 1000])
def test_stale_sets_and_their_readers(dev, k, B):
    """After k lazy row-split steps only the row-split images follow the parameters; inr_forward validates the forward
    images, inr_backward the transposed ones -- each time the buffer moves towards a full pack of the same parameters
    (a second plan's) and ends equal to it byte for byte.  Then the other way round: k plain steps, and inr_train_step
    (which reads, and moves no parameter) under INR_RS=1 as the reader of the row-split images."""
    from inr_mi355x import _lib as L
    with env(INR_LAZY_PACK="1", INR_RS=None):
        model, enc, eng = make(dev, 256, 3)
        _, _, full = make(dev, 256, 3)
        x, gt = data(dev, B)
        assert state(eng) == (L.IMG_ALL, 1)
        for _ in range(k):
            step(eng, enc, x, gt, "1")
        assert state(eng)[0] == L.IMG_RS
        full.params.copy_(eng.params)
        full.pack()  # (its own plan: a pack tells a plan that every set of ITS buffer is valid)
        want = full.packed.view(torch.int32)
        got = lambda: eng.packed.view(torch.int32)
        d0 = got() != want
        assert int(d0.sum()) > 0  # the forward and transposed images were left behind
        out = eng.forward(x, enc.B, save=True)
        assert state(eng)[0] == L.IMG_RS | L.IMG_FWD
        d1 = got() != want
        assert int(d1.sum()) < int(d0.sum()) and not bool((d1 & ~d0).any())  # one set caught up, nothing else moved
        eng.backward(x, enc.B, torch.ones_like(out))
        assert state(eng)[0] == L.IMG_ALL
        assert torch.equal(got(), want)
        # the other family
        for _ in range(k):
            step(eng, enc, x, gt, "0")
        assert state(eng)[0] == L.IMG_FWD | L.IMG_TR
        full.params.copy_(eng.params)
        full.pack()
        assert int((got() != want).sum()) > 0
        with env(INR_RS="1"):
            eng.train_step(x, enc.B, gt, spec())
        assert state(eng)[0] == L.IMG_ALL
        assert torch.equal(got(), want)


def clearing_run(dev, lazy):
    from inr_mi355x import checkpoint
    with env(INR_LAZY_PACK=lazy, INR_RS=None):
        model, enc, eng = make(dev, 256, 3)
        x, gt = data(dev, 127)
        cfg = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=1e-4)
        losses = [step(eng, enc, x, gt, "1"), step(eng, enc, x, gt, "1")]
        ckpt = checkpoint.save_dict(model, enc, eng, cfg)  # a save reads the parameters, not the images
        losses.append(step(eng, enc, x, gt, "1"))
        checkpoint.load_dict(model, enc, eng, ckpt)  # back to step 2: writes the parameters, then packs
        packed_after_load, valid_after_load = eng.packed.clone(), state(eng)[0]
        losses.append(step(eng, enc, x, gt, "0"))  # a plain step right after the load
        losses.append(step(eng, enc, x, gt, "1"))
        eng.pack()  # explicit pack in mid-sequence
        valid_after_pack = state(eng)[0]
        losses.append(step(eng, enc, x, gt, "0"))
        out = eng.forward(x, enc.B).clone()
        torch.cuda.synchronize()
        return dict(losses=losses, params=eng.params.clone(), m1=eng.exp_avg.clone(), m2=eng.exp_avg_sq.clone(), out=out,
                    packed_after_load=packed_after_load, valid=(valid_after_load, valid_after_pack), step=eng.step)


def test_pack_clearing_paths(dev):
    from inr_mi355x import _lib as L
    lazy, eager = clearing_run(dev, "1"), clearing_run(dev, "0")
    assert lazy["valid"] == (L.IMG_ALL, L.IMG_ALL) == eager["valid"]
    assert lazy["step"] == eager["step"] == 5
    assert [x.hex() for x in lazy["losses"]] == [x.hex() for x in eager["losses"]]
    for k in ("params", "m1", "m2", "out", "packed_after_load"):
        same_bits(lazy[k], eager[k], k)
