"""The helper kernels against the bits of a named commit's library (``-m gpu``).  tests/golden/aux_bits.json holds, per
case of tests/aux_bits_cases.py, the SHA-256 of every output buffer as the library built from ``producer_commit`` wrote
it (tools/make_golden.py aux_bits; recorded twice, cases that differed between the two runs left out).  Slab reduction,
Adam, re-pack, penalties, losses, encoders, shuffle and the metric / display / band / coil reductions all sum in a fixed
order, so a later library reproduces every hash or has changed what these kernels compute."""
import json
import os

import pytest

import aux_bits_cases as A

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aux_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert len(GOLDEN["producer_commit"]) == 40
    assert GOLDEN["not_deterministic"] == []
    assert sorted(GOLDEN["cases"]) == sorted(A.CASES)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_bits_match_producer(name):
    want = GOLDEN["cases"][name]
    got = A.run_case(name)
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    assert not wrong, f"{name}: {len(wrong)} of {len(want)} buffers differ from {GOLDEN['producer_commit'][:7]}: {wrong[:8]}"
