"""tests/golden/host_layout.json replayed against the built library (CPU only: creating and sizing a plan touches no GPU).
The table was recorded by tools/make_golden.py host_layout from the library of the commit it names -- before the host layer
learnt to derive a call's layout once -- so launch dims, workspace sizes, step info, return codes and error texts of every
plan x batch size x INR_RS x INR_OVERLAP (x INR_GEMM_ONE_CLASS at creation, bf16) are held to what that commit answered."""
import json
import os

import pytest

import layout_table as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_layout.json")


@pytest.fixture(scope="module")
def table():
    with open(GOLD) as f:
        t = json.load(f)
    assert len(t["producer_commit"]) == 40
    # the recorder and this replay ask the same questions
    assert t["B"] == T.B_VALUES and [tuple(s) for s in t["switches"]] == T.SWITCHES
    assert (t["desc_fields"], t["sizes_fields"], t["info_fields"]) == (T.DESC_FIELDS, T.SIZES_FIELDS, T.INFO_FIELDS)
    t["plans"] = T.unpack(t)
    return t


def test_table_covers_what_it_should(table):
    from inr_mi355x import _lib as L
    plans = table["plans"]
    assert len(plans) >= 200 and all(len(p["rows"]) == len(T.B_VALUES) for p in plans if p["create"][0] == 0)
    ok = [p for p in plans if p["create"][0] == 0]
    assert any(p["create"][0] != 0 for p in plans)
    assert {p["desc"]["depth"] for p in ok if p["desc"]["precision"] == L.PRECISION_BF16} >= {3, 5, 8}
    assert any(p["one_class"] for p in ok)
    blocks = lambda p: p["rows"][1]["sw"][0][1][1 + T.INFO_FIELDS.index("hidden_blocks")]
    assert any(p["desc"]["kind"] == L.KIND_WIRE and blocks(p) == 12 for p in ok)
    assert any(p["desc"]["kind"] == L.KIND_WIRE2D and blocks(p) == 16 for p in ok)
    for inp in (L.INPUT_GAUSS, L.INPUT_X):
        assert any(p["desc"]["kind"] == L.KIND_MSFOURIER and p["desc"]["width"] == 512 and p["desc"]["input"] == inp for p in ok)
    # the switches do matter somewhere: row-split plans follow INR_RS, split steps follow INR_OVERLAP
    assert any(len(r["sw"]) == len(T.SWITCHES) for p in ok for r in p["rows"])


def test_every_record_replays(table, monkeypatch):
    from inr_mi355x import _lib as L
    for k in ("INR_RS", "INR_OVERLAP", "INR_GEMM_ONE_CLASS", "INR_GEMM_ENC_COST"):
        monkeypatch.delenv(k, raising=False)
    n = 0
    for want in table["plans"]:
        got = T.plan_record(L, want["desc"], want["one_class"])
        if got != want:  # name the first field that differs
            assert got["create"] == want["create"], want["desc"]
            assert got["sizes"] == want["sizes"], want["desc"]
            for B, g, w in zip(T.B_VALUES, got["rows"], want["rows"]):
                assert g == w, (want["desc"], want["one_class"], B)
        n += len(T.B_VALUES) * len(T.SWITCHES)
    assert n == len(table["plans"]) * len(T.B_VALUES) * len(T.SWITCHES)
