"""Weight images on demand, the rules only (CPU: creating a plan touches no GPU): which image sets are valid after a pack,
an update and a read, which sets each network call reads, and what a plan reports before its first call."""
import ctypes as C
import itertools

import pytest


@pytest.fixture(scope="module")
def lib():
    from inr_mi355x import _lib as L
    return L.load()


def test_transitions(lib):
    from inr_mi355x import _lib as L
    after = lib.inr_image_sets_after
    every = range(L.IMG_ALL + 1)
    for valid, sets in itertools.product(every, every):
        # an update: the parameters moved, only what it wrote is current -- whatever was valid before
        assert after(valid, L.IMG_EV_UPDATE, sets) == sets
        # a pack and the re-pack in front of a read add their sets and drop none
        assert after(valid, L.IMG_EV_PACK, sets) == valid | sets
        assert after(valid, L.IMG_EV_READ, sets) == valid | sets
    for valid in every:
        assert after(valid, L.IMG_EV_PACK, L.IMG_ALL) == L.IMG_ALL  # a full pack clears every flag
        assert after(valid, L.IMG_EV_UPDATE, L.IMG_ALL) == L.IMG_ALL  # so does an eager update
        assert after(valid, L.IMG_EV_UPDATE, 0xF8 | L.IMG_RS) == L.IMG_RS  # bits that name no set are ignored


def test_what_each_call_reads(lib):
    from inr_mi355x import _lib as L
    read = lib.inr_image_sets_read
    assert read(L.IMG_CALL_STEP, 1) == L.IMG_RS
    assert read(L.IMG_CALL_STEP, 0) == L.IMG_FWD | L.IMG_TR
    for rs in (0, 1):  # forward and backward run inr_mlp_kernel whatever INR_RS says
        assert read(L.IMG_CALL_FORWARD, rs) == L.IMG_FWD
        assert read(L.IMG_CALL_BACKWARD, rs) == L.IMG_FWD | L.IMG_TR
    # a row-split step and a plain step validate disjoint sets: alternating them re-packs every time
    assert read(L.IMG_CALL_STEP, 1) & read(L.IMG_CALL_STEP, 0) == 0
    # the step sequences of the GPU test, replayed on the rules: update leaves the step's own sets, a read adds its own
    valid = L.IMG_ALL
    for rs in (1, 0, 1):
        reads = read(L.IMG_CALL_STEP, rs)
        valid = lib.inr_image_sets_after(valid, L.IMG_EV_READ, reads & ~valid)
        assert valid & reads == reads
        valid = lib.inr_image_sets_after(valid, L.IMG_EV_UPDATE, reads)
        assert valid == reads
    valid = lib.inr_image_sets_after(valid, L.IMG_EV_READ, read(L.IMG_CALL_FORWARD, 0) & ~valid)
    assert valid == L.IMG_RS | L.IMG_FWD


def _plan(lib, width, enc):
    from inr_mi355x import _lib as L
    desc = L.NetDesc(kind=L.KIND_SIREN, in_features=2 * enc, width=width, depth=3, out_features=2, last_act=L.ACT_ID,
                     input=L.INPUT_GAUSS, enc_size=enc, w0=30.0, first_omega_0=0.0, hidden_omega_0=0.0, scale_0=0.0,
                     precision=L.PRECISION_F32)
    plan = C.c_void_p()
    L.check(lib.inr_plan_create(C.byref(desc), C.byref(plan)))
    return plan


def _state(lib, plan):
    from inr_mi355x import _lib as L
    valid, lazy = C.c_int32(-1), C.c_int32(-1)
    L.check(lib.inr_plan_image_sets(plan, C.byref(valid), C.byref(lazy)))
    return valid.value, lazy.value


def test_plan_state_before_any_call(lib, monkeypatch):
    from inr_mi355x import _lib as L
    monkeypatch.delenv("INR_LAZY_PACK", raising=False)
    rs_plan, plain = _plan(lib, 256, 32), _plan(lib, 64, 32)
    try:
        info = L.StepInfo()
        monkeypatch.setenv("INR_RS", "1")
        L.check(lib.inr_plan_step_info(rs_plan, 1000, C.byref(info)))
        assert info.row_split == 1
        L.check(lib.inr_plan_step_info(plain, 1000, C.byref(info)))
        assert info.row_split == 0  # one kernel, one image family: nothing to be lazy about
        assert _state(lib, rs_plan) == (L.IMG_ALL, 0)  # opt-in: unset means eager
        assert _state(lib, plain) == (L.IMG_ALL, 0)
        monkeypatch.setenv("INR_LAZY_PACK", "1")  # read per call
        assert _state(lib, rs_plan) == (L.IMG_ALL, 1)
        assert _state(lib, plain) == (L.IMG_ALL, 0)
        monkeypatch.setenv("INR_LAZY_PACK", "0")
        assert _state(lib, rs_plan) == (L.IMG_ALL, 0)
        assert lib.inr_plan_image_sets(rs_plan, None, None) != 0  # null argument: an error, not a crash
    finally:
        lib.inr_plan_destroy(rs_plan)
        lib.inr_plan_destroy(plain)
