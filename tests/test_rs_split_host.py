"""The split row-split step, the schedule only (CPU: creating a plan touches no GPU): where inr_plan_step_split says a
step with gradients runs as a 256-tile first launch + a remainder launch beside two weight-gradient GEMM parts, the two
launches deal every column block once, the two GEMM parts every stash slot once, and everything that runs side by side
has a CU of its own.  Plans: the graded 5 x 256 behind gauss-256 (the shape the split is for) and a depth-3 / gauss-32
plan (the model, calibrated on the graded plan's kernels alone, prices its GEMM shorter than a remainder launch and never
engages it: other depths are unmeasured and stay on the single launch)."""
import ctypes as C

import pytest

NT_MAX = 2048


@pytest.fixture(scope="module")
def lib():
    from inr_mi355x import _lib as L
    return L.load()


def _plan(lib, depth, enc):
    from inr_mi355x import _lib as L
    desc = L.NetDesc(kind=L.KIND_SIREN, in_features=2 * enc, width=256, depth=depth, out_features=2, last_act=L.ACT_ID,
                     input=L.INPUT_GAUSS, enc_size=enc, w0=30.0, first_omega_0=0.0, hidden_omega_0=0.0, scale_0=0.0,
                     precision=L.PRECISION_F32)
    plan = C.c_void_p()
    L.check(lib.inr_plan_create(C.byref(desc), C.byref(plan)))
    return plan


@pytest.fixture(scope="module")
def table(lib):
    """per plan: {nt: (split words, StepInfo fields, n_slabs of inr_plan_workspace)} under the default switches"""
    import os
    from inr_mi355x import _lib as L
    saved = {k: os.environ.pop(k, None) for k in ("INR_RS", "INR_OVERLAP")}
    out = {}
    try:
        for key in ((5, 256), (3, 32)):
            plan = _plan(lib, *key)
            rows = {}
            for nt in range(1, NT_MAX + 1):
                w = (C.c_int64 * L.STEP_SPLIT_WORDS)()
                L.check(lib.inr_plan_step_split(plan, nt * 128, w))
                info = L.StepInfo()
                L.check(lib.inr_plan_step_info(plan, nt * 128, C.byref(info)))
                slots, slabs = C.c_int64(), C.c_int64()
                L.check(lib.inr_plan_workspace(plan, nt * 128, C.byref(slots), C.byref(slabs)))
                rows[nt] = (list(w), (info.row_split, info.ncb, info.grid, info.rounds, info.hi, info.lo, info.n_hi),
                            slabs.value)
            lib.inr_plan_destroy(plan)
            out[key] = rows
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return out


def _blocks(blk0, hi, lo, n_hi, grid):
    """the column blocks a one-round launch deals, as (first, count) per workgroup"""
    out = []
    for t in range(grid):
        n = hi if t < n_hi else lo
        first = blk0 + (t * hi if t < n_hi else n_hi * hi + (t - n_hi) * lo)
        out.append((first, n))
    return out


def test_engaged_layouts_are_partitions(table):
    n_engaged = 0
    for rows in table.values():
        for nt, (w, info, slabs) in rows.items():
            assert w[15] == slabs
            if not w[0]:
                assert w[:15] == [0] * 15
                continue
            n_engaged += 1
            (_, lo1, hi, lo, n_hi, n_rem, ncb, a_end, a_tpc, a_chunks, a_wgs, b0, b_tpc, b_chunks, b_wgs, n_slabs) = w
            # the two launches deal every column block of [0, 8 nt) exactly once, in legal tiles
            assert 1 <= lo1 <= 7 and 1 <= ncb <= 7 and hi == ncb and (lo == hi or (lo % 2 == 0 and 0 < lo < hi))
            assert 1 <= n_hi <= n_rem
            dealt = _blocks(0, lo1, lo1, 256, 256) + _blocks(256 * lo1, hi, lo, n_hi, n_rem)
            assert all(n >= 1 for _, n in dealt)
            covered = sorted(b for first, n in dealt for b in range(first, first + n))
            assert covered == list(range(8 * nt)), nt
            # A's and B's chunks deal every slot exactly once; A inside the first launch, B over all the remainder touches
            assert a_end == 256 * lo1 // 8 == b0 and 256 * lo1 % 8 == 0
            assert (a_chunks - 1) * a_tpc < a_end <= a_chunks * a_tpc
            assert (b_chunks - 1) * b_tpc < nt - b0 <= b_chunks * b_tpc
            rem_slots = {b // 8 for first, n in dealt[256:] for b in range(first, first + n)}
            assert rem_slots == set(range(b0, nt))
            # side by side: GEMM part A and the remainder launch; then part B where the remainder was
            assert a_wgs >= a_chunks >= 1 and b_wgs >= b_chunks >= 1
            assert a_wgs + n_rem <= 256 and b_wgs <= n_rem
            # slabs: the grid's, then A's chunks, then B's
            assert n_slabs >= 256 + a_chunks + b_chunks
    assert n_engaged > 0


def test_where_it_never_engages(table):
    for rows in table.values():
        for nt, (w, info, _) in rows.items():
            row_split, ncb, grid, rounds, hi, lo, n_hi = info
            if nt < 128 or (8 * nt) % 256 == 0 or not row_split or rounds != 1 or grid != 256:
                assert w[0] == 0, nt
            if w[0]:  # the single launch it replaces: one round, some tiles a block wider than lo1
                assert (row_split, grid, rounds) == (1, 256, 1) and ncb == w[1] + 1 and 8 * nt // 256 >= 4
    assert table[(5, 256)][160][0][0] == 0  # 1280 blocks = 256 x 5: no remainder
    assert all(w[0] == 0 for w, _, _ in table[(3, 32)].values())  # (modelled, not measured: excluded on the safe side)


def test_graded_shape_engages(lib, table, monkeypatch):
    from inr_mi355x import _lib as L
    rows = table[(5, 256)]
    for nt in (129, 161, 196):
        assert rows[nt][0][0] == 1, nt
    # 25 000 rows: six blocks on every workgroup, 32 one-block tiles beside part A's 220 workgroups, part B on 20
    assert rows[196][0][:15] == [1, 6, 1, 1, 32, 32, 1, 192, 9, 22, 220, 192, 2, 2, 20]
    assert rows[196][1] == (1, 7, 256, 1, 7, 6, 32)  # inr_plan_step_info goes on describing the single launch
    assert rows[196][2] == 256 + 25  # ... whose 25 GEMM chunks still set the workspace (A + B: 24)
    # INR_OVERLAP=0 and INR_RS=0, read per call, select the single launch; the workspace follows neither
    plan = _plan(lib, 5, 256)
    try:
        for name in ("INR_OVERLAP", "INR_RS"):
            monkeypatch.setenv(name, "0")
            w = (C.c_int64 * L.STEP_SPLIT_WORDS)()
            L.check(lib.inr_plan_step_split(plan, 25000, w))
            assert list(w) == [0] * 15 + [256 + 25]
            monkeypatch.delenv(name)
        w = (C.c_int64 * L.STEP_SPLIT_WORDS)()
        L.check(lib.inr_plan_step_split(plan, 25000, w))
        assert w[0] == 1
        assert lib.inr_plan_step_split(plan, 0, w) != 0 and lib.inr_plan_step_split(plan, 25000, None) != 0
    finally:
        lib.inr_plan_destroy(plan)
