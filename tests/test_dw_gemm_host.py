"""tests/dw_gemm_cases.py checked without a GPU (creating a plan touches none): the float64 restatement against
torch.autograd through oracle.*_forward, element by element at 1e-12 x S; the fp32 restatement's own error e_ref finite and
positive for every case and layer (the criterion FACTOR x e_ref is not vacuous); the chunking rule restated there against
the chunk count inr_plan_workspace reports, for every case; ids unique and seeds taken from them; and the table reaching
every instantiation of the GEMM.  tests/test_gpu_dw_gemm.py holds the kernels to the same references."""
import math

import pytest
import torch

import dw_gemm_cases as D

# the references of the large batches (grid, wbm4, split) are formed once here and once on the device run: dense only
IDS = [c.id for c in D.CASES]


@pytest.fixture(scope="module")
def table():
    """per case id: (prep, operands)"""
    return {c.id: (D.prepare(c.shape), D.operands(D.prepare(c.shape), c)) for c in D.CASES}


def test_ids_are_unique_and_seed_the_case():
    assert len(set(IDS)) == len(IDS)
    assert len({c.seed for c in D.CASES}) == len(D.CASES)
    c = next(k for k in D.CASES if k.B == "base" and k.pattern == "zeros")
    p = D.prepare(c.shape)
    a, b = D.operands(p, c), D.operands(p, c)
    assert torch.equal(a.x, b.x) and torch.equal(a.dout, b.dout)
    other = D.operands(p, D.Case(c.shape, 1, "base", "spread"))   # same shape and batch, another id: other numbers
    assert other.x.shape == a.x.shape and not torch.equal(other.x, a.x)


def test_shapes_land_on_the_builds_they_name():
    for s in D.SHAPES.values():
        p = D.prepare(s.name)
        eng = p.engine
        assert eng.step_save_by_tile, s.name
        assert eng.tile_rows == s.TL, (s.name, eng.tile_rows)
        nb = D.step_info(eng, 1).hidden_blocks
        assert nb == int(s.build[2:]) and (3 if nb == 12 else 4) == s.WB, (s.name, nb)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_reference_is_autograd_in_float64_and_e_ref_is_positive(table, case):
    p, o = table[case.id]
    r64, r32 = D.reference(p, o, torch.float64), D.reference(p, o, torch.float32)
    auto = D.autograd_reference(p, o)
    assert [r.name for r in r64] == p.layers
    ys = D.yardstick(p, o, case, r64, r32)
    for a, b, g, (ew, eb) in zip(r64, r32, auto, ys):
        assert torch.isfinite(a.g).all() and torch.isfinite(a.S).all() and bool((a.S >= 0).all())
        assert bool(((a.g - g).abs() <= 1e-12 * a.S).all()), (case.id, a.name, float(((a.g - g).abs() / a.S.clamp_min(1e-300)).max()))
        assert D.err(b.g, a)[2], (case.id, a.name)
        if case.pattern == "allzero":   # nothing to scale by: the criterion there is the exact zero alone
            assert not bool(a.S.any()) and not bool(b.g.any())
            continue
        assert math.isfinite(ew) and ew > 0 and math.isfinite(eb) and eb > 0, (case.id, a.name, ew, eb)
        # and the bound stays a bound: a dropped, doubled or misplaced term moves a one-term sum by S itself (err = 1), so
        # FACTOR x e_ref has to stay well below 1.  (Many-term sums sit at 1e-7; a one-term sum carries the relative error
        # of a single act' next to its zero crossing -- 1e-3 for SIREN's cos(30 z), 2e-2 for WIRE's Gabor factor in fp32.)
        assert D.FACTOR * ew < 0.5 and D.FACTOR * eb < 0.5, (case.id, a.name, ew, eb)


def test_db_allowance_is_the_sincos_bound_and_only_where_the_loss_forms_dout():
    from sincos_cases import BOUND_CW
    assert BOUND_CW == 3.8e-7
    for c in D.CASES:
        assert D.db_allowance(c) == (2 * BOUND_CW if c.route in (2, 3) else 0.0), c.id


def test_onehot_rows_leave_one_term_sums(table):
    """dZ is non-zero at the chosen coordinate alone, in every covered layer"""
    n = 0
    for c in D.CASES:
        if c.pattern != "onehot":
            continue
        p, o = table[c.id]
        for r in D.reference(p, o, torch.float64):
            rows = r.dZ.abs().sum(1).nonzero().reshape(-1).tolist()
            assert rows == [o.row], (c.id, r.name, rows[:4])
        n += 1
    assert n > 0


def test_altsign_bias_sums_cancel(table):
    for c in D.CASES:
        if c.pattern != "altsign":
            continue
        p, o = table[c.id]
        for r in D.reference(p, o, torch.float64):
            b = r.is_bias
            live = b & (r.S > 0)
            assert bool(live.any())
            # what is left is the last, unpaired row alone -- a few percent of S_b where a per-tensor norm sees nothing else
            assert bool(((r.g[b] - r.dZ[o.B - 1]).abs() <= 1e-12 * r.S[b]).all()), c.id
            assert float((r.g[live].abs() / r.S[live]).max()) < 0.1, c.id


def _grid_and_split_chunks(p, B):
    """workgroups of the widest fused launch and chunks of the split row-split step, whatever the switches say"""
    nt, nb = D._dims(p.engine, B)
    with D._env(INR_RS="1", INR_OVERLAP=None):
        rs_plan = bool(D.step_info(p.engine, B).row_split)
        w = D.step_split(p.engine, B)
    grid = max(nb, min(p.engine.max_blocks, 8 * nt)) if rs_plan else nb
    return grid, (w[9] + w[13] if w[0] else 0), rs_plan


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_restated_chunking_matches_the_workspace(table, case):
    """n_slabs = the fused grid + the most chunks any route of the batch stores: the restated rule must give that count
    with the overlap switch on (plain, the split step's two parts, the split row-split step's) and off (plain alone)"""
    p, o = table[case.id]
    B = o.B
    grid, rs_chunks, rs_plan = _grid_and_split_chunks(p, B)
    plain = D.plain_launch(p, B)
    with D._env(INR_RS="0", INR_OVERLAP=None):
        step = D.step_launches(p, D.Case(case.shape, 2, case.B), B)
        n_on = p.engine.workspace(B)[1]
    with D._env(INR_RS="0", INR_OVERLAP="0"):
        n_off = p.engine.workspace(B)[1]
    assert n_off == grid + max(plain.chunks, rs_chunks), (case.id, n_off, grid, plain, rs_chunks)
    assert n_on == grid + max(plain.chunks, sum(l.chunks for l in step), rs_chunks), (case.id, n_on, grid, plain, step)
    if rs_chunks <= plain.chunks and p.shape.split_kernel and case.B in ("ragged", "grid", "wbm4"):
        # the other tile height would have stored another number of slabs: from chunks of two tiles on, the reported count
        # tells WBM = 2 from WBM = 4 (below, one tile a chunk either way, the rule alone says which)
        items, mb = D.items_of(p), p.engine.max_blocks
        other = D._chunk_tiles(plain.tile1, mb // D._units(items, 6 - plain.wbm, 4))[1]
        assert other != plain.chunks, (case.id, plain, other)
    for l in o.launches:   # every chunk has tiles (inr_layout.hip chunk_tiles leaves none empty), every tile one chunk
        assert (l.chunks - 1) * l.tpc < l.tile1 - l.tile0 <= l.chunks * l.tpc
    assert o.launches[0].tile0 == 0 and o.launches[-1].tile1 == D._dims(p.engine, B)[0]
    assert all(a.tile1 == b.tile0 for a, b in zip(o.launches, o.launches[1:]))


def test_every_instantiation_has_a_case(table):
    """the four fp32 shapes, the three-term kernel on both tile heights, a launch with tile0 > 0, ragged chunks"""
    seen = set()
    for c in D.CASES:
        p, o = table[c.id]
        s = p.shape
        for l in o.launches:
            ragged = (l.tile1 - l.tile0) % l.tpc != 0
            if s.split_kernel:
                seen |= {("split", l.wbm), ("f32", 128, l.wbm, 4)}   # (every such case runs under INR_DW_SPLIT=0 too)
                seen.add(("place", "on")), seen.add(("place", "off"))
            else:
                seen.add(("f32", s.TL, l.wbm, s.WB))
            if l.tile0 > 0:
                seen.add(("tile0", s.TL, s.WB, c.route))
            if ragged:
                seen.add(("ragged", s.TL, s.WB))
            if l.chunks >= 2:
                seen.add(("chunks2", s.TL, s.WB))
    want = {("f32", 128, 4, 4), ("f32", 128, 2, 4), ("f32", 64, 4, 4), ("f32", 64, 3, 3), ("split", 2), ("split", 4),
            ("place", "on"), ("place", "off"), ("tile0", 128, 4, 3), ("tile0", 128, 4, 2), ("tile0", 64, 4, 2),
            ("tile0", 64, 3, 2), ("ragged", 128, 4), ("ragged", 64, 4), ("ragged", 64, 3), ("chunks2", 128, 4),
            ("chunks2", 64, 4), ("chunks2", 64, 3)}
    assert want <= seen, want - seen
    # square tiles over more than one slot (the stage loop crossing a tile boundary with WBM = 4) have their own case
    p, o = table["siren256-r1-Bwbm4-dense"]
    assert o.launches[0].wbm == 4 and o.launches[0].tpc * p.engine.tile_rows >= 1024 and o.launches[0].chunks >= 2
