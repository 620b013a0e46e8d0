"""The split row-split step on the GPU (``-m gpu``): csrc/inr_layout.hip rs_split_schedule, csrc/inr_api.hip run_fused_step.

A row-split step with gradients whose single launch is one round with a few tiles one column block wider than the rest
runs as a 256-tile first launch, then a remainder launch beside part A of the weight-gradient GEMM, then part B.  Every
check runs both settings in one process on one plan: INR_OVERLAP=0 (the single launch; read per call) against the default.

  * the stash is computed per coordinate: bitwise equal over all slots;
  * tiles and K-chunks group coordinates differently, so the last layer's sums, the loss and the GEMM's chunk sums move
    in their last bits.  Gradients: per weight tensor, relative L2 error against the float64 oracle e_split (default) and
    e_one (single launch); required  e_split <= max(2 e_one, 1e-6)  -- the criterion of tests/test_gpu_dw_split.py --
    and 1e-5 against the fp32 oracle.  Loss: rtol 1e-5 between the settings, the bar tests/test_gpu_rs.py sets between
    the two fused kernels;
  * two split calls are bitwise equal in gradients, loss and slabs; inr_train_adam_step equals inr_train_step +
    inr_adam_step bitwise;
  * every measured call starts from a workspace filled with NaN (stash slots, slabs, gradients), and one case steps the
    parameters first and checks against the oracle at the new ones: what a call reads it must have written itself, in
    the order the fork and the join set -- an earlier call's correct bits cannot stand in.

The plan is the graded SIREN 5 x 256 behind gauss-256: the schedule's model is calibrated on that plan's kernels only and
engages no depth-3 plan (unmeasured there, excluded on the safe side; tests/test_rs_split_host.py).  The measured pairs go through conftest.record_parity
(profiles/rs_split_parity.jsonl is a committed copy)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402  (checker only)

DEPTH, WIDTH, E = 5, 256, 256
# name: (rows, engaged)
SHAPES = {
    "nt129_ragged": (129 * 128 - 5, True),  # the smallest engaged shape; the ragged last slot lies in the remainder
    "graded_25000": (25000, True),          # 32 one-block tiles behind 256 tiles of 6
    "nt161": (161 * 128, True),             # lo1 = 5
    "nt160": (160 * 128, False),            # 1280 blocks = 256 x 5: no remainder, nothing to split
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class _single_launch:
    """INR_OVERLAP=0 for the calls inside."""

    def __enter__(self):
        self.old = os.environ.get("INR_OVERLAP")
        os.environ["INR_OVERLAP"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["INR_OVERLAP"]
        else:
            os.environ["INR_OVERLAP"] = self.old


def _engaged(eng, B):
    from inr_mi355x import _lib as L
    w = (C.c_int64 * L.STEP_SPLIT_WORDS)()
    L.check(eng.lib.inr_plan_step_split(eng.plan, B, w))
    return bool(w[0])


def _bits(t):
    return t.view(torch.int32).clone()


def _poison(eng, n_save, n_slab):
    """NaN over the stash slots and the slabs of the batch, and over the gradient and loss words"""
    eng._save[:n_save].fill_(float("nan"))
    eng._slabs[:n_slab].fill_(float("nan"))
    eng.grads.fill_(float("nan"))
    torch.cuda.synchronize()


def _setup(dev, B, seed, masked=False):
    import inr_mi355x as M
    net = dict(network_input_size=2 * E, network_output_size=2, network_depth=DEPTH, network_width=WIDTH)
    enc_cfg = dict(embedding="gauss", scale=2, embedding_size=E, coordinates_size=3)
    torch.manual_seed(seed)
    enc = M.Positional_Encoder(enc_cfg, device=dev)
    mdl = M.SIREN(net)
    sd = {k: v.clone() for k, v in mdl.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    coords = torch.rand(B, 3, generator=g) * 2 - 1
    gt = torch.randn(B, 2, generator=g) * 0.3
    mask = torch.rand(B, generator=g) < 0.6 if masked else None
    return M, net, enc, mdl, sd, coords, gt, mask


def _oracle(sd, net, coords, enc_B, gt, mask, dtype):
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = O.siren_forward(params, O.encode(coords.to(dtype), enc_B.to(dtype), "gauss"), net)
    o, g = (out, gt.to(dtype)) if mask is None else (out[mask], gt.to(dtype)[mask])
    loss = O.loss_l2_half(o, g)
    grads = torch.autograd.grad(loss, list(params.values()))
    return torch.cat([x.reshape(-1) for x in grads]), loss.detach()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _run_both(dev, name, masked=False):
    """one plan, one batch: the single launch, then the default twice.  Returns everything the checks look at."""
    from inr_mi355x import _lib as L
    B, engaged = SHAPES[name]
    M, net, enc, mdl, sd, coords, gt, mask = _setup(dev, B, 17 + B % 97, masked)
    mdl = mdl.to(dev)
    eng = mdl.fused_engine(E)
    cd, gd, encB = coords.to(dev), gt.to(dev), enc.B.contiguous()
    md = None if mask is None else mask.to(torch.uint8).to(dev)
    cnt = B if mask is None else int(mask.sum())
    spec = M.LossSpec(L.LOSS_L2_HALF)
    nt = (B + 127) // 128
    n_save = nt * eng.save_floats_per_tile
    n_slab = eng.workspace(B)[1] * eng.slab_floats

    eng.train_step(cd, encB, gd, spec, count=cnt, mask=md)  # (the workspace exists from here on)

    def step():
        # every measured call starts from a poisoned workspace: a slot or slab the call reads without having written it
        # (a remainder launch that skips its slots, a GEMM part that runs ahead of the launch it depends on, a reduction
        # ahead of the join) puts NaN into the stash comparison, the gradients or the loss instead of the previous
        # call's correct bits
        _poison(eng, n_save, n_slab)
        loss = eng.train_step(cd, encB, gd, spec, count=cnt, mask=md).clone()
        torch.cuda.synchronize()
        return dict(loss=loss.cpu(), grads=eng.grads.clone().cpu(), stash=_bits(eng._save[:n_save]),
                    slabs=_bits(eng._slabs[:n_slab]))

    assert _engaged(eng, B) == engaged, name
    with _single_launch():
        assert not _engaged(eng, B)
        one = step()
    split = step()
    again = step()
    # (the large buffers are compared here and dropped: only the verdicts are kept for the tests that share this run)
    for a, b in ((split, one), (split, again)):
        for k in ("stash", "slabs"):
            b[k + "_equal"] = bool(torch.equal(a[k], b[k]))
    for d in (one, split, again):
        del d["stash"], d["slabs"]
    return dict(B=B, engaged=engaged, sd=sd, net=net, coords=coords, gt=gt, mask=mask, encB=enc.B.cpu(), one=one,
                split=split, again=again)


_cache = {}


def _case(dev, name, masked=False):
    key = (name, masked)
    if key not in _cache:
        _cache[key] = _run_both(dev, name, masked)
    return _cache[key]


@pytest.mark.parametrize("name", list(SHAPES))
def test_stash_bitwise_and_deterministic(dev, name):
    r = _case(dev, name)
    assert r["one"]["stash_equal"], "the stash must not change by a bit"
    for k in ("loss", "grads"):  # two identical calls
        assert torch.equal(r["split"][k], r["again"][k]), k
    assert r["again"]["stash_equal"] and r["again"]["slabs_equal"]
    torch.testing.assert_close(r["split"]["loss"], r["one"]["loss"], rtol=1e-5, atol=0)
    if not r["engaged"]:  # the same launches under both settings: bitwise equal throughout
        for k in ("loss", "grads"):
            assert torch.equal(r["split"][k], r["one"][k]), k
        assert r["one"]["slabs_equal"]


def _check_gradients(tag, r):
    from conftest import record_parity
    ref64, loss64 = _oracle(r["sd"], r["net"], r["coords"], r["encB"], r["gt"], r["mask"], torch.float64)
    ref32, _ = _oracle(r["sd"], r["net"], r["coords"], r["encB"], r["gt"], r["mask"], torch.float32)
    # (poisoned workspace: a NaN anywhere fails here; the loss against the oracle's, the bar of tests/test_gpu_rs.py)
    assert torch.isfinite(r["split"]["grads"]).all() and torch.isfinite(r["one"]["grads"]).all()
    torch.testing.assert_close(r["split"]["loss"].double(), loss64, rtol=1e-5, atol=0)
    at = 0
    for k, v in r["sd"].items():
        n = v.numel()
        e_split = _rel(r["split"]["grads"][at:at + n], ref64[at:at + n])
        e_one = _rel(r["one"]["grads"][at:at + n], ref64[at:at + n])
        record_parity("rs_split:" + tag, what=k, e_split=e_split, e_one=e_one)
        print(f"rs_split:{tag} {k}: e_split {e_split:.3e} e_one {e_one:.3e}")
        assert e_split <= max(2 * e_one, 1e-6), (tag, k, e_split, e_one)
        at += n
    assert at == ref64.numel()
    assert _rel(r["split"]["grads"], ref32) < 1e-5, (tag, _rel(r["split"]["grads"], ref32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_against_float64(dev, name):
    _check_gradients(name, _case(dev, name))


def test_gradients_masked_loss(dev):
    r = _case(dev, "nt129_ragged", masked=True)
    assert r["one"]["stash_equal"]
    torch.testing.assert_close(r["split"]["loss"], r["one"]["loss"], rtol=1e-5, atol=0)
    _check_gradients("nt129_ragged-masked", r)


@pytest.mark.parametrize("name", ["nt129_ragged", "graded_25000"])
def test_one_call_equals_two_calls(dev, name):
    """inr_train_adam_step (the update rides in the reduction's launch) against inr_train_step + inr_adam_step, both split"""
    from inr_mi355x import _lib as L
    B, _ = SHAPES[name]
    M, net, enc, mdl, sd, coords, gt, _ = _setup(dev, B, 5)
    cd, gd, encB = coords.to(dev), gt.to(dev), enc.B.contiguous()
    spec = M.LossSpec(L.LOSS_L2_HALF)
    res = []
    for one_call in (True, False):
        m = M.SIREN(net)
        m.load_state_dict(sd)
        eng = m.to(dev).fused_engine(E)
        assert _engaged(eng, B)
        for _ in range(2):
            if one_call:
                loss = eng.train_adam_step(cd, encB, gd, spec, 1e-3).clone()
            else:
                loss = eng.train_step(cd, encB, gd, spec).clone()
                eng.adam_step(1e-3)
        torch.cuda.synchronize()
        res.append([_bits(t).cpu() for t in (loss.reshape(1), eng.grads, eng.params, eng.exp_avg, eng.exp_avg_sq, eng.packed)])
    for a, b, what in zip(res[0], res[1], ("loss", "grads", "params", "exp_avg", "exp_avg_sq", "packed")):
        assert torch.equal(a, b), what


def test_against_float64_after_the_parameters_moved(dev):
    """The calls above repeat one batch on one set of parameters.  Here two split Adam steps move the parameters first, the
    workspace is poisoned, and the next step's gradients and loss are held to the float64 oracle AT THE NEW PARAMETERS:
    stash slots, slabs or weight images left over from an earlier call cannot stand in for this call's own."""
    from inr_mi355x import _lib as L
    name = "nt129_ragged"
    B, _ = SHAPES[name]
    M, net, enc, mdl, sd, coords, gt, _ = _setup(dev, B, 23)
    eng = mdl.to(dev).fused_engine(E)
    cd, gd, encB = coords.to(dev), gt.to(dev), enc.B.contiguous()
    spec = M.LossSpec(L.LOSS_L2_HALF)
    assert _engaged(eng, B)
    for _ in range(2):
        eng.train_adam_step(cd, encB, gd, spec, 1e-3)
    torch.cuda.synchronize()
    flat = eng.params.detach().cpu().clone()
    sd2, at = {}, 0
    for k, v in sd.items():
        sd2[k] = flat[at:at + v.numel()].reshape(v.shape).clone()
        at += v.numel()
    assert at == flat.numel() and not all(torch.equal(sd2[k], sd[k]) for k in sd)
    n_save = ((B + 127) // 128) * eng.save_floats_per_tile
    n_slab = eng.workspace(B)[1] * eng.slab_floats
    res = {}
    for key in ("split", "one"):
        _poison(eng, n_save, n_slab)
        if key == "one":
            with _single_launch():
                loss = eng.train_step(cd, encB, gd, spec).clone()
        else:
            loss = eng.train_step(cd, encB, gd, spec).clone()
        torch.cuda.synchronize()
        res[key] = dict(loss=loss.cpu(), grads=eng.grads.clone().cpu())
    _check_gradients(name + "-moved", dict(sd=sd2, net=net, coords=coords, gt=gt, mask=None, encB=enc.B.cpu(), **res))
