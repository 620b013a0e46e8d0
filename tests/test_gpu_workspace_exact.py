"""A fused step writes inside the workspace inr_plan_workspace reports, and nowhere else (``-m gpu``).

The engine is handed a stash and a slab buffer of EXACTLY the reported extents -- views into larger tensors with 4096
sentinel floats in front and behind -- for every way a step lays out its launches: in-kernel weight gradients, the
row-split kernel, the plain fused kernel, the split step with the side stream and without it, 64-coordinate tiles, the
mask-driven reduction of the wide filter network, and the bf16 kernels with one and two chunk classes.  Structural and
bitwise throughout: sentinels intact, finite loss and gradients, two steps on the same inputs bit-equal."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -12345.678

# (id, family, width, precision, B, INR_RS, INR_OVERLAP); depth 3 behind a gauss encoder of 32 unless the family says otherwise
PATHS = [
    ("inkernel-w32", "SIREN", 32, "f32", 300, None, None),        # in-kernel dW, stash by block
    ("rowsplit", "SIREN", 256, "f32", 300, None, None),           # row-split: more workgroups (24) than slots (3)
    ("plain", "SIREN", 256, "f32", 300, "0", None),               # inr_mlp_kernel + batch GEMM
    ("split", "SIREN", 256, "f32", 38400, "0", None),             # 300 slots = 256 + 44: side stream
    ("split-off", "SIREN", 256, "f32", 38400, "0", "0"),
    ("wire-nb12", "WIRE", 256, "f32", 19200, None, None),         # 64-coordinate tiles, 300 of them, split step
    ("mfn-512", "MultiscaleKFourier", 512, "f32", 200, None, None),  # depth 1: mask-driven reduction
    ("bf16", "SIREN", 256, "bf16", 300, None, None),
    ("bf16-two-classes", "SIREN", 256, "bf16", 38400, None, None),   # two tiles per workgroup, two chunk classes
]


def _guarded(n, dev, fill):
    """a view of exactly n floats between two guards of sentinels"""
    big = torch.full((n + 2 * GUARD,), SENTINEL, device=dev)
    view = big[GUARD:GUARD + n]
    if fill is not None:
        view.fill_(fill)
    return big, view


def _guards_intact(big, n):
    want = torch.full((GUARD,), SENTINEL, device=big.device)
    return torch.equal(big[:GUARD], want) and torch.equal(big[GUARD + n:], want)


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_step_stays_inside_the_reported_workspace(path, monkeypatch):
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    from inr_mi355x import mfn
    _, family, width, precision, B, rs, overlap = path
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    for k, v in (("INR_RS", rs), ("INR_OVERLAP", overlap)):  # (monkeypatch restores both)
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, v)
    torch.manual_seed(0)
    enc = M.Positional_Encoder(dict(embedding="gauss", scale=1, embedding_size=32, coordinates_size=3), device=dev)
    encB, kw = enc.B.contiguous(), {}
    g = torch.Generator().manual_seed(B + width)
    coords = (torch.rand(B, 3, generator=g) * 2 - 1).to(dev)
    gt = (torch.randn(B, 2, generator=g) * 0.2).to(dev)
    if family == "SIREN":
        model = M.SIREN(dict(network_input_size=64, network_output_size=2, network_depth=3, network_width=width)).to(dev)
        eng = model.fused_engine(32, precision)
    elif family == "WIRE":
        model = M.WIRE(dict(network_input_size=3, network_output_size=2, network_depth=3, network_width=width,
                            first_omega_0=10, hidden_omega_0=10, scale=5)).to(dev)
        eng, encB = model._engine(), None
    else:
        model = mfn.MultiscaleKFourier(dict(network_input_size=64, network_output_size=2, network_depth=1,
                                            network_width=width)).to(dev)
        model.bind_encoder(enc)
        eng = model._engine("gauss")
        kw = dict(dist=torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2).contiguous())
    # the path this case is here for
    nt, nb = eng.launch_dims(B)
    slots, n_slabs = eng.workspace(B)
    info = L.StepInfo()
    L.check(eng.lib.inr_plan_step_info(eng.plan, B, C.byref(info)))
    assert eng.step_save_by_tile == (path[0] != "inkernel-w32")
    assert info.row_split == (path[0] == "rowsplit") and (path[0] != "rowsplit" or info.grid > nt)
    if path[0] in ("split", "split-off", "wire-nb12"):
        assert (nt, nb) == (300, 256)
        with monkeypatch.context() as m:
            m.setenv("INR_OVERLAP", "0")
            unsplit = eng.workspace(B)[1]
        assert (n_slabs > unsplit) == (overlap is None), "the split step has its own chunk slabs"
    if path[0] == "bf16-two-classes":
        assert (nt, nb) == (300, 150)
    n_save, n_slab = slots * eng.save_floats_per_tile, n_slabs * eng.slab_floats
    big_save, eng._save = _guarded(n_save, dev, 0.0)  # (the engine's own stash starts as zeros)
    big_slab, eng._slabs = _guarded(n_slab, dev, None)
    grads = []
    for _ in range(2):
        loss = eng.train_step(coords, encB, gt, M.LossSpec(L.LOSS_L2_HALF), **kw)
        torch.cuda.synchronize()
        assert eng._save.data_ptr() == big_save.data_ptr() + 4 * GUARD and eng._save.numel() == n_save
        assert eng._slabs.data_ptr() == big_slab.data_ptr() + 4 * GUARD and eng._slabs.numel() == n_slab
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(eng.grads).all())
        grads.append(eng.grads.clone())
    assert _guards_intact(big_save, n_save), "a step wrote outside its stash"
    assert _guards_intact(big_slab, n_slab), "a step wrote outside its slabs"
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    assert bool((grads[0] != 0).any())
