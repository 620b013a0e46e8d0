"""The weight-gradient GEMM on the bf16 matrix pipe (csrc/inr_dw_gemm_split.hip): every fp32 operand as three bf16
terms hi + mid + lo (truncation split), six of the nine partial products, fp32 accumulation.

Accuracy criterion (GPU tests): per weight tensor, the relative L2 error against the oracle's gradients evaluated in
float64 is e_split with the new kernel and e_f32 with the fp32 kernel (INR_DW_SPLIT=0, read per call: same process,
same plan); required is  e_split <= max(2 e_f32, 1e-6)  -- the factor 2 is the allowance for the dropped 2^-24 terms on
top of one rounding per accumulate -- together with the project's 1e-5 bar against the fp32 oracle.  Two calls on the
same inputs are bitwise equal.  The measured pairs are appended through conftest.record_parity
(profiles/dw_split_parity.jsonl is a committed copy)."""
import os

import numpy as np
import pytest
import torch

import oracle as O  # noqa: E402  (checker only)


# ---- the split itself, restated in numpy (no GPU) ---------------------------------------------------------------------
def split3(x):
    """hi = x & 0xffff0000, r = x - hi, mid = r & 0xffff0000, lo = r - mid (float32 arithmetic throughout)."""
    x = np.asarray(x, dtype=np.float32)
    hi = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = x - hi
    mid = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    lo = r - mid
    return hi, mid, lo


def test_split_is_exact_on_cpu():
    rng = np.random.default_rng(0)
    n = 1_000_000
    bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32).copy()
    x[~np.isfinite(x)] = 1.0
    # the smallest normals (their remainders are subnormal), the largest finite values, plain magnitudes, special ones
    x[:1000] = (np.uint32(0x00800000) + rng.integers(0, 1 << 16, 1000).astype(np.uint32)).view(np.float32)
    x[1000:2000] = (np.uint32(0x7F7F0000) + rng.integers(0, 1 << 16, 1000).astype(np.uint32)).view(np.float32)
    x[2000:300000] = rng.standard_normal(298000).astype(np.float32)
    x[300000:300003] = np.array([0.0, 1e-30, 1e4], dtype=np.float32)
    hi, mid, lo = split3(x)
    assert np.array_equal(((hi + mid) + lo).view(np.uint32), x.view(np.uint32))
    mz = split3(np.float32(-0.0))  # (-0 comes back as hi = -0, mid = lo = +0: the same value)
    assert mz[0] == 0 and mz[1] == 0 and mz[2] == 0
    # each term fits bf16: nothing below the upper 16 bits.  (From |x| >= 2^-102 on: below, mid or lo are fp32 subnormals, whose
    # bits no longer line up with bf16's -- the sum above is still exact, the planes then drop less than 2^-133.)
    big = np.abs(x) >= 2.0 ** -102
    for term in (hi, mid, lo):
        assert not np.any(term[big].view(np.uint32) & np.uint32(0xFFFF))
    # the six products kept leave out a2 b3 + a3 b2 + a3 b3.  Truncation to 8 significant bits leaves |a2| < 2^-7 |a| and
    # |a3| < 2^-15 |a|, so the rigorous bound is 2 x 2^-22 + 2^-30 < 2^-21 |a b|; typical terms are 2^-8 and 2^-16 of a, which
    # puts the typical omission at 2^-24 |a b|: one fp32 rounding.
    a, b = x[2000:300000:2].astype(np.float64), x[2001:300000:2].astype(np.float64)
    (a1, a2, a3), (b1, b2, b3) = [t.astype(np.float64) for t in split3(a)], [t.astype(np.float64) for t in split3(b)]
    kept = a1 * b1 + a1 * b2 + a2 * b1 + a2 * b2 + a1 * b3 + a3 * b1
    assert np.all(np.abs(kept - a * b) <= 2.0 ** -21 * np.abs(a * b))
    assert np.mean(np.abs(kept - a * b) / np.abs(a * b)) <= 2.0 ** -24


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _fp32_kernel:
    """INR_DW_SPLIT=0 for the calls inside."""

    def __enter__(self):
        self.old = os.environ.get("INR_DW_SPLIT")
        os.environ["INR_DW_SPLIT"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["INR_DW_SPLIT"]
        else:
            os.environ["INR_DW_SPLIT"] = self.old


def _per_tensor(flat, sd):
    out, at = {}, 0
    for k, v in sd.items():
        out[k] = flat[at:at + v.numel()].double()
        at += v.numel()
    assert at == flat.numel()
    return out


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _compare(tag, sd, g_split, g_f32, ref64, ref32):
    """e_split <= max(2 e_f32, 1e-6) per tensor, 1e-5 against the fp32 oracle; returns the largest ratio."""
    from conftest import record_parity
    worst = 0.0
    ts, tf, t64 = _per_tensor(g_split, sd), _per_tensor(g_f32, sd), _per_tensor(ref64, sd)
    for k in sd:
        e_split, e_f32 = _rel(ts[k], t64[k]), _rel(tf[k], t64[k])
        record_parity("dw_split:" + tag, what=k, e_split=e_split, e_f32=e_f32)
        print(f"dw_split:{tag} {k}: e_split {e_split:.3e} e_f32 {e_f32:.3e}")
        assert e_split <= max(2 * e_f32, 1e-6), (tag, k, e_split, e_f32)
        worst = max(worst, e_split / max(e_f32, 1e-300))
    if ref32 is not None:
        assert _rel(g_split, ref32) < 1e-5, (tag, _rel(g_split, ref32))
    return worst


def _oracle(sd, net, coords, enc_B, dtype, loss_fn):
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = O.siren_forward(params, O.encode(coords.to(dtype), enc_B.to(dtype), "gauss"), net)
    grads = torch.autograd.grad(loss_fn(out), list(params.values()))
    return torch.cat([g.reshape(-1) for g in grads])


def _setup(dev, width, depth, E, B, seed):
    import inr_mi355x as M
    net = dict(network_input_size=2 * E, network_output_size=2, network_depth=depth, network_width=width)
    enc_cfg = dict(embedding="gauss", scale=2, embedding_size=E, coordinates_size=3)
    torch.manual_seed(seed)
    enc = M.Positional_Encoder(enc_cfg, device=dev)
    mdl = M.SIREN(net)
    sd = {k: v.clone() for k, v in mdl.state_dict().items()}
    mdl = mdl.to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    coords = torch.rand(B, 3, generator=g) * 2 - 1
    gt = torch.randn(B, 2, generator=g) * 0.3
    return M, net, enc, mdl, sd, coords, gt


def _fused_pair(eng, step, differ=True):
    """gradients of the fused step with the new kernel (twice: bitwise equal) and with the fp32 kernel"""
    step()
    g_split = eng.grads.clone()
    step()
    assert torch.equal(eng.grads, g_split)
    with _fp32_kernel():
        step()
        g_f32 = eng.grads.clone()
    if differ:  # (the switch does select another kernel; a handful of coordinates may round alike)
        assert not torch.equal(g_split, g_f32)
    return g_split.cpu(), g_f32.cpu()


# B: one partial slot | a slot boundary (127, 129) | a ragged last chunk | several K-chunks with the half-height tiles
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 127, 129, 1000, 4133])
@pytest.mark.parametrize("depth,E", [(3, 32), (3, 256), (5, 32), (5, 256)])
def test_siren_l2(dev, depth, E, B):
    from inr_mi355x import _lib as L
    M, net, enc, mdl, sd, coords, gt = _setup(dev, 256, depth, E, B, 100 * depth + E)
    eng = mdl.fused_engine(E)
    assert eng.step_save_by_tile
    cd, gd, encB = coords.to(dev), gt.to(dev), enc.B.contiguous()
    g_split, g_f32 = _fused_pair(eng, lambda: eng.train_step(cd, encB, gd, M.LossSpec(L.LOSS_L2_HALF)), differ=B >= 1000)
    loss = lambda out: O.loss_l2_half(out, gt.to(out.dtype))  # noqa: E731
    ref64 = _oracle(sd, net, coords, enc.B.cpu(), torch.float64, loss)
    ref32 = _oracle(sd, net, coords, enc.B.cpu(), torch.float32, loss)
    _compare(f"siren256-d{depth}-E{E}-B{B}", sd, g_split, g_f32, ref64, ref32)


@pytest.mark.gpu
def test_masked_hdr(dev):
    """Rows outside the mask have dZ = 0 in every layer: all-zero operand rows next to ordinary ones."""
    B, E = 1000, 32
    M, net, enc, mdl, sd, coords, gt = _setup(dev, 256, 3, E, B, 7)
    opts = dict(hdr_eps=1e-3, hdr_ff_sigma=2, hdr_ff_factor=0.5)
    mask = torch.rand(B, generator=torch.Generator().manual_seed(3)) < 0.6
    f = torch.exp(-(coords[:, 1] ** 2 + coords[:, 2] ** 2) / (2 * 2.0 ** 2))
    A = float(torch.mean((1 - f) ** 2))
    spec = M.LossSpec.from_config({"loss": "HDR", "loss_opts": opts})
    eng = mdl.fused_engine(E)
    cd, gd, md, encB = coords.to(dev), gt.to(dev), mask.to(torch.uint8).to(dev), enc.B.contiguous()
    g_split, g_f32 = _fused_pair(
        eng, lambda: eng.train_step(cd, encB, gd, spec, count=int(mask.sum()), mask=md, hdr_A=A))
    loss = lambda out: O.loss_hdr(out[mask], gt.to(out.dtype)[mask], coords.to(out.dtype), opts)[0]  # noqa: E731
    ref64 = _oracle(sd, net, coords, enc.B.cpu(), torch.float64, loss)
    # (the HDR loss divides by |y| + eps: its fp32 evaluation is itself far from float64, so no fp32-oracle bar here)
    _compare("masked-hdr-B1000", sd, g_split, g_f32, ref64, None)


@pytest.mark.gpu
def test_width_160_padded_rows(dev):
    from inr_mi355x import _lib as L
    B, E = 1000, 32
    M, net, enc, mdl, sd, coords, gt = _setup(dev, 160, 3, E, B, 11)
    eng = mdl.fused_engine(E)
    assert eng.step_save_by_tile
    cd, gd, encB = coords.to(dev), gt.to(dev), enc.B.contiguous()
    g_split, g_f32 = _fused_pair(eng, lambda: eng.train_step(cd, encB, gd, M.LossSpec(L.LOSS_L2_HALF)))
    loss = lambda out: O.loss_l2_half(out, gt.to(out.dtype))  # noqa: E731
    ref64 = _oracle(sd, net, coords, enc.B.cpu(), torch.float64, loss)
    ref32 = _oracle(sd, net, coords, enc.B.cpu(), torch.float32, loss)
    _compare("siren160-d3-E32-B1000", sd, g_split, g_f32, ref64, ref32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed", "tiny_only"])
def test_special_operands(dev, case):
    """Forward / backward pair with a chosen d(loss)/d(out): rows of zeros (masked rows: dZ = 0 in every layer), one entry
    at 1e-30 and one at 1e+4 -- dZ spans 34 decades and the split must carry each magnitude; `tiny_only`: nothing but
    the 1e-30 entry, so that it is not hidden behind the large ones."""
    B, E = 300, 32
    M, net, enc, mdl, sd, coords, gt = _setup(dev, 256, 3, E, B, 13)
    dout = torch.randn(B, 2, generator=torch.Generator().manual_seed(5)) * 1e-3
    dout[100:200] = 0.0
    if case == "tiny_only":
        dout[:] = 0.0
    dout[7, 1] = 1e-30
    if case == "mixed":
        dout[250, 0] = 1e4
    eng = mdl._engine()
    x = enc.embedding(coords.to(dev)).contiguous()

    def run():
        eng.forward(x, None, save=True)
        return eng.backward(x, None, dout.to(dev)).clone()

    g_split = run()
    assert torch.equal(run(), g_split)
    with _fp32_kernel():
        g_f32 = run()
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    out = O.siren_forward(params, O.encode(coords.double(), enc.B.cpu().double(), "gauss"), net)
    ref64 = torch.cat([g.reshape(-1) for g in torch.autograd.grad(out, list(params.values()), grad_outputs=dout.double())])
    assert torch.isfinite(g_split).all()
    _compare("special-" + case, sd, g_split.cpu(), g_f32.cpu(), ref64, None)
