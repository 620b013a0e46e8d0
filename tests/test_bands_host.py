"""Radial band statistics on the host (inr_mi355x/bands.py): band_stats_numpy -- the definition the
kernel is held to -- against a literal per-band boolean-mask loop in torch; overlapping, nested and empty bands, the
mask halves, pred=None; the report's err_db / None rules, the table, --band-report's parsing and the header's
declarations.  None of it touches a GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

from inr_mi355x import _lib as L
from inr_mi355x import bands as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_FIELDS, EXACT_FIELDS = ("energy", "sse"), ("n", "max_abs2", "max_comp", "min_comp", "max_err2")


def _field(C=2, H=32, W=24, seed=0):
    """A random [C*H*W,2] field and prediction over the (y, x) grid of a C x H x W scan, with its radius."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(-1, 1, H).reshape(1, H, 1).expand(C, H, W)
    x = torch.linspace(-1, 1, W).reshape(1, 1, W).expand(C, H, W)
    dist = torch.sqrt(y ** 2 + x ** 2).reshape(-1).contiguous()
    gt = torch.randn(C * H * W, 2, generator=g) * torch.exp(-3 * dist).reshape(-1, 1)
    pred = gt + 0.05 * torch.randn(C * H * W, 2, generator=g)
    return dist, gt.contiguous(), pred.contiguous()


def _torch_loop(dist, gt, pred, bounds, take=None):
    """The literal statement: per band a boolean mask, then torch reductions (fp64 sums of fp64 terms)."""
    out = []
    for r0, r1 in bounds:
        sel = (dist >= r0) & (dist <= r1)  # fp32 tensor against a Python float: compared in fp32
        if take is not None:
            sel = sel & take
        g = gt[sel]
        row = {"n": float(sel.sum()), "energy": float((g.double() ** 2).sum(dim=-1).sum()), "sse": 0.0,
               "max_abs2": -math.inf, "max_comp": -math.inf, "min_comp": math.inf, "max_err2": -math.inf}
        if g.shape[0]:
            row["max_abs2"] = float((g ** 2).sum(dim=-1).max())
            row["max_comp"], row["min_comp"] = float(g.abs().max()), float(g.abs().min())
        if pred is not None:
            e = ((pred[sel].double() - g.double()) ** 2).sum(dim=-1)
            row["sse"] = float(e.sum())
            if g.shape[0]:
                row["max_err2"] = float(e.max())
        out.append(row)
    return out


def _assert_matches(st, rows, n_total):
    tol = 2.0 * n_total * 2.0 ** -53  # reordering n non-negative fp64 terms
    for b, row in enumerate(rows):
        for f in EXACT_FIELDS:
            assert getattr(st, f)[b] == row[f], (b, f, getattr(st, f)[b], row[f])
        for f in SUM_FIELDS:
            assert abs(getattr(st, f)[b] - row[f]) <= tol * abs(row[f]), (b, f, getattr(st, f)[b], row[f])


def test_numpy_matches_torch_loop_on_rings_with_boundary_rows():
    dist, gt, pred = _field()
    bounds = B.ring_bounds(8)
    # rows exactly on shared boundaries: the fp32 value of ring 2's / ring 5's upper end
    edge = [np.float32(bounds[2][1]), np.float32(bounds[5][1])]
    dist[100], dist[777] = float(edge[0]), float(edge[1])
    assert float(dist[100]) == float(np.float32(bounds[3][0]))
    st = B.band_stats_numpy(dist, gt, pred, bounds=bounds)
    _assert_matches(st, _torch_loop(dist, gt, pred, bounds), dist.numel())
    # a boundary row counts in both rings: every row lies in some ring, the two edge rows in two
    inside = int(((dist >= 0) & (dist <= math.sqrt(2))).sum())
    shared = sum(int(((dist >= bounds[i][0]) & (dist <= bounds[i][1]) & (dist >= bounds[i + 1][0])
                      & (dist <= bounds[i + 1][1])).sum()) for i in range(7))
    assert shared >= 2 and int(st.n.sum()) == inside + shared
    for ring, row in ((2, 100), (3, 100), (5, 777), (6, 777)):
        one = B.band_stats_numpy(dist[row:row + 1], gt[row:row + 1], bounds=bounds)
        assert one.n[ring] == 1.0
    assert st.lo.dtype == np.float32 and st.n.dtype == np.float64


def test_overlapping_nested_empty_and_uncovered():
    dist, gt, pred = _field(seed=1)
    bounds = [(0.0, 0.5), (0.25, 0.75), (0.3, 0.4), (0.41, 0.41000001), (3.0, 4.0), (0.0, 0.9)]  # rows beyond 0.9: uncovered
    st = B.band_stats_numpy(dist, gt, pred, bounds=bounds)
    _assert_matches(st, _torch_loop(dist, gt, pred, bounds), dist.numel())
    assert st.n[4] == 0 and st.energy[4] == 0 and st.sse[4] == 0
    assert st.max_abs2[4] == -math.inf and st.max_comp[4] == -math.inf and st.max_err2[4] == -math.inf
    assert st.min_comp[4] == math.inf
    assert st.n[2] < st.n[0] and st.n[2] < st.n[1] and st.n[5] < dist.numel()


def test_mask_halves_sum_to_the_whole_and_pred_none():
    dist, gt, pred = _field(seed=2)
    bounds = B.ring_bounds(8)
    mask = (torch.rand(dist.numel(), generator=torch.Generator().manual_seed(3)) < 0.3).to(torch.uint8) * 7
    whole = B.band_stats_numpy(dist, gt, pred, bounds=bounds)
    a = B.band_stats_numpy(dist, gt, pred, mask=mask, mask_select=1, bounds=bounds)
    b = B.band_stats_numpy(dist, gt, pred, mask=mask, mask_select=0, bounds=bounds)
    _assert_matches(a, _torch_loop(dist, gt, pred, bounds, take=mask != 0), dist.numel())
    _assert_matches(b, _torch_loop(dist, gt, pred, bounds, take=mask == 0), dist.numel())
    assert np.array_equal(a.n + b.n, whole.n)
    for f in SUM_FIELDS:
        assert np.allclose(getattr(a, f) + getattr(b, f), getattr(whole, f), rtol=1e-12, atol=0)
    assert np.array_equal(np.maximum(a.max_comp, b.max_comp), whole.max_comp)
    assert np.array_equal(np.minimum(a.min_comp, b.min_comp), whole.min_comp)
    none = B.band_stats_numpy(dist, gt, None, bounds=bounds)
    assert np.all(none.sse == 0) and np.all(none.max_err2 == -math.inf)
    assert np.array_equal(none.energy, whole.energy) and np.array_equal(none.max_abs2, whole.max_abs2)


def test_bad_bounds_are_refused():
    dist, gt, _ = _field()
    for bounds in ([], [(0.0, 1.0)] * 65, [(0.5, 0.25)], [(float("nan"), 1.0)]):
        with pytest.raises(ValueError):
            B.band_stats_numpy(dist, gt, bounds=bounds)


def _stats(n, energy, sse, max_err2):
    K = len(n)
    z = np.zeros(K)
    return B.BandStats(np.arange(K, dtype=np.float32), np.arange(1, K + 1, dtype=np.float32), np.asarray(n, float),
                       np.asarray(energy, float), np.asarray(sse, float), z, z, z, np.asarray(max_err2, float))


def test_report_rules():
    rep = B.band_report(_stats([10, 0, 5, 4], [2.0, 0.0, 0.0, 8.0], [0.02, 0.0, 1.0, 0.0],
                               [0.01, -math.inf, 0.25, -math.inf]))
    assert [set(r) for r in rep] == [{"lo", "hi", "n", "energy", "sse", "err_db", "max_abs_err"}] * 4
    assert rep[0]["err_db"] == pytest.approx(-20.0) and rep[0]["max_abs_err"] == pytest.approx(0.1)
    assert rep[0]["n"] == 10 and rep[0]["lo"] == 0.0 and rep[0]["hi"] == 1.0
    assert rep[1]["err_db"] is None and rep[1]["max_abs_err"] is None  # an empty band
    assert rep[2]["err_db"] is None and rep[2]["max_abs_err"] == 0.5  # rows without energy
    assert rep[3]["err_db"] == -math.inf and rep[3]["max_abs_err"] is None  # no prediction / an exact fit


def test_table_format():
    rep = B.band_report(_stats([10, 0], [2.0, 0.0], [0.02, 0.0], [0.01, -math.inf]))
    lines = B.format_band_table(rep).split("\n")
    assert lines[0] == B.REPORT_TITLE
    assert lines[1].split() == ["ring", "lo", "hi", "n", "energy", "err", "dB", "max", "|err|"]
    assert set(lines[2].replace(" ", "")) == {"-"}
    assert lines[3].split() == ["0", "0", "1", "10", "2", "-20", "0.1"]
    assert lines[4].split() == ["1", "1", "2", "0", "0", "n/a", "n/a"]
    assert len(lines) == 5
    assert B.format_band_table(rep, "T").split("\n")[0] == "T"


def test_report_bounds():
    assert B.report_bounds(None) == B.ring_bounds(40) and B.report_bounds(True, 8) == B.ring_bounds(8)
    assert B.report_bounds(5) == B.ring_bounds(5)
    assert B.report_bounds([(0, 0.5), (0.25, 1)]) == [(0.0, 0.5), (0.25, 1.0)]
    assert B.flag_bounds(None) is None and B.flag_bounds(0) is True and B.flag_bounds(12) == 12
    for bad in (65, 0, [(0.0, 1.0)] * 65, [(0.5, 0.25)], []):
        with pytest.raises(ValueError):
            B.report_bounds(bad)


def test_print_band_tables(capsys):
    from inr_mi355x.cli import print_band_tables
    print_band_tables({"psnr": 1.0})
    assert capsys.readouterr().out == ""
    rep = B.band_report(_stats([10], [2.0], [0.02], [0.01]))
    print_band_tables({"bands": rep, "bands_sampled": rep, "bands_unsampled": rep})
    out = capsys.readouterr().out.split("\n")
    titles = [l for l in out if l.startswith(B.REPORT_TITLE)]
    assert titles == [B.REPORT_TITLE, B.REPORT_TITLE + ", sampled rows", B.REPORT_TITLE + ", unsampled rows"]
    assert out == (B.format_band_table(rep) + "\n" + B.format_band_table(rep, titles[1]) + "\n"
                   + B.format_band_table(rep, titles[2]) + "\n").split("\n")


def test_cli_band_report_parsing(tmp_path, capsys):
    from inr_mi355x import reconstruct
    from inr_mi355x.cli import parse_cli
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model: SIREN\n")
    base = ["--config", str(cfg)]
    assert parse_cli(argv=base)[0].band_report is None
    assert parse_cli(argv=base + ["--val", "--band-report"])[0].band_report == 0
    assert parse_cli(argv=base + ["--val", "--band-report", "12"])[0].band_report == 12
    assert parse_cli(False, argv=base + ["--band-report", "6"])[0].band_report == 6  # the ring loop needs no --val
    for bad in (base + ["--band-report"], base + ["--val", "--band-report", "65"], base + ["--val", "--band-report", "0"],
                base + ["--val", "--band-report", "x"]):
        with pytest.raises(SystemExit):
            parse_cli(argv=bad)
    rbase = base + ["--checkpoint", "x.pt", "--synthetic", "2,8,8"]
    assert reconstruct.parse_args(rbase + ["--compare"]).band_report is None
    assert reconstruct.parse_args(rbase + ["--compare", "--band-report"]).band_report == 0
    assert reconstruct.parse_args(rbase + ["--compare", "--band-report", "8"]).band_report == 8
    with pytest.raises(SystemExit):
        reconstruct.parse_args(rbase + ["--band-report"])
    assert "--band-report needs --compare" in capsys.readouterr().err


def test_header_declares_both_entries():
    with open(os.path.join(ROOT, "include", "inr_abi.h")) as f:
        text = f.read()
    assert re.search(r"^int inr_band_stats_scratch\(int64_t n, int32_t n_bands, int64_t\* scratch_doubles\);", text, re.M)
    assert re.search(r"^int inr_band_stats\(const float\* dist, const float\* gt, const float\* pred, const uint8_t\* mask,",
                     text, re.M)
    macros = dict(re.findall(r"^#define (INR_BAND_\w+) (\d+)", text, re.M))
    assert int(macros["INR_BAND_FIELDS"]) == L.BAND_FIELDS == len(B.FIELDS) == len(B.BandStats._fields) - 2
    assert int(macros["INR_BAND_MAX"]) == L.BAND_MAX == 64
    assert int(macros["INR_BAND_TILE_ROWS"]) == L.BAND_TILE_ROWS
    assert "inr_band_stats" in L.SYMBOLS and "inr_band_stats_scratch" in L.SYMBOLS
    assert len(L.SYMBOLS["inr_band_stats"][1]) == 12
