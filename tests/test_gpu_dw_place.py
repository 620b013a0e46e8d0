"""Placement of the weight-gradient GEMM's workgroups (csrc/inr_dw_place.h, dw_gemm_split_kernel): a chunk's
workgroups are handed block ids 8 apart, which share an XCD's L2.  The map only changes WHICH block computes a piece of
work, so the flat gradient of a fused step is bitwise what it is with INR_DW_PLACE=0 (block-id order; read per call).

Per case: a step on other inputs, the step with the placement on (g_on), a step on other inputs, the step with
INR_DW_PLACE=0 (g_off), a step on other inputs, the step with the placement on again.  The steps in between overwrite
every slab with other values: a piece of work that no workgroup took would otherwise still find the identical result of
the previous call in its slab.  Required: g_on == g_off == the second g_on, bitwise.

Cases: the smallest shapes that reach each form of the grid (G workgroups; the map treats G < 8, G % 8 != 0, a short
last chunk, another number of workgroups per chunk and more than one round of the chip's 256 CUs differently).  The
grid follows from dw_gemm_chunk / dw_gemm_units (csrc/inr_layout.hip, csrc/inr_dw_gemm.hip), restated in _grid below."""
import os

import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _in_id_order:
    """INR_DW_PLACE=0 for the calls inside."""

    def __enter__(self):
        self.old = os.environ.get("INR_DW_PLACE")
        os.environ["INR_DW_PLACE"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["INR_DW_PLACE"]
        else:
            os.environ["INR_DW_PLACE"] = self.old


def _grid(depth, E, B):
    """(workgroups of the GEMM launch, workgroups per chunk) of a SIREN of hidden width <= 256 with a gauss encoder of
    size E: items = layer 0 (8 x 2E/32 blocks of 32 rows) and layers 1 .. depth - 2 (8 x 8), 256 x 256 tiles, or
    128 x 256 ones when a chunk would hold under 1024 coordinates; the kernel runs two workgroups per 256 x 256 tile."""
    nt = (B + 127) // 128

    def chunking(wbm):
        units = 0
        for kblk in [2 * E // 32] + [8] * (depth - 2):
            units += ((8 + 2 * wbm - 1) // (2 * wbm)) * ((kblk + 7) // 8)
        target = max(1, 256 // units)
        tpc = (nt + target - 1) // target
        return units, tpc, (nt + tpc - 1) // tpc

    units, tpc, n_chunks = chunking(4)
    if nt > 1 and tpc * 128 < 1024:
        units, tpc, n_chunks = chunking(2)
        return n_chunks * units, units
    return n_chunks * units * 2, units * 2


# width, depth, E, B, the grid the case is there for (None: whatever follows)
CASES = [
    (256, 3, 32, 1, 4),        # G < 8: one tile, two workgroups per 256 x 256 tile
    (256, 5, 256, 1, 10),      # G < 16, G % 8 = 2
    (256, 5, 256, 129, 20),    # two chunks of 128 x 256 tiles
    (256, 5, 256, 1000, 80),   # G % 8 = 0
    (256, 5, 256, 4133, 170),  # a short last chunk, G % 8 = 2
    (256, 3, 32, 4133, None),  # another number of workgroups per chunk
    (160, 3, 32, 1000, None),  # rows past a tensor's extent
    (256, 5, 256, 36000, 240),  # two rounds of the fused kernel; the GEMM's chunks still take 128 x 256 tiles: one round
    (256, 5, 256, 46000, 450),  # the chunks are long enough for 256 x 256 tiles again: more than one round of 256 workgroups
]


@pytest.mark.gpu
@pytest.mark.parametrize("width,depth,E,B,grid", CASES)
def test_placement_is_bitwise_neutral(dev, width, depth, E, B, grid):
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    G, bpc = _grid(depth, E, B)
    print(f"dw_place: width {width} depth {depth} E {E} B {B}: grid {G} = {G // bpc} chunks x {bpc} workgroups, G % 8 = {G % 8}")
    if grid is not None:
        assert G == grid
    net = dict(network_input_size=2 * E, network_output_size=2, network_depth=depth, network_width=width)
    enc_cfg = dict(embedding="gauss", scale=2, embedding_size=E, coordinates_size=3)
    torch.manual_seed(1000 * depth + E + B)
    enc = M.Positional_Encoder(enc_cfg, device=dev)
    mdl = M.SIREN(net).to(dev)
    g = torch.Generator().manual_seed(B)
    coords, gt = (torch.rand(B, 3, generator=g) * 2 - 1).to(dev), (torch.randn(B, 2, generator=g) * 0.3).to(dev)
    coords2, gt2 = (torch.rand(B, 3, generator=g) * 2 - 1).to(dev), (torch.randn(B, 2, generator=g) * 0.3).to(dev)
    encB = enc.B.contiguous()
    eng = mdl.fused_engine(E)
    assert eng.step_save_by_tile  # (the plan takes its weight gradients from the batch GEMM)
    spec = M.LossSpec(L.LOSS_L2_HALF)

    def step(c, y):
        eng.train_step(c, encB, y, spec)
        return eng.grads.clone()

    g_other = step(coords2, gt2)
    g_on = step(coords, gt)
    assert not torch.equal(g_on, g_other)
    step(coords2, gt2)
    with _in_id_order():
        g_off = step(coords, gt)
    step(coords2, gt2)
    g_on2 = step(coords, gt)
    assert torch.isfinite(g_on).all()
    assert torch.equal(g_on, g_off)
    assert torch.equal(g_on, g_on2)
