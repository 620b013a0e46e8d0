"""One refused call into each host translation unit of the C-ABI -- inr_plan.hip, inr_layout.hip, inr_api.hip,
inr_api_offgrid.hip and inr_api_aux.hip -- read back through inr_last_error: every file writes the one error text, and the
text is the calling thread's own.  CPU only: each call is refused before anything is launched."""
import ctypes as C
import threading

import pytest


@pytest.fixture(scope="module")
def L():
    from inr_mi355x import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def siren(L):
    d = L.NetDesc(kind=L.KIND_SIREN, in_features=16, width=32, depth=4, out_features=2, last_act=L.ACT_TANH,
                  input=L.INPUT_GAUSS, enc_size=8, w0=30.0)
    plan = C.c_void_p()
    assert L.load().inr_plan_create(C.byref(d), C.byref(plan)) == 0, L.last_error()
    yield plan
    L.load().inr_plan_destroy(plan)


def test_plan_file(L, siren):
    d = L.NetDesc(kind=99, in_features=16, width=32, depth=4, out_features=2, input=L.INPUT_GAUSS, enc_size=8)
    plan = C.c_void_p()
    assert L.load().inr_plan_create(C.byref(d), C.byref(plan)) != 0
    assert L.last_error() == "inr_plan_create: kind 99 has no kernel yet"


def test_layout_file(L, siren):
    a, b = C.c_int64(), C.c_int64()
    assert L.load().inr_plan_launch_dims(siren, 0, C.byref(a), C.byref(b)) != 0
    assert L.last_error() == "inr_plan_launch_dims: B = 0"


def test_network_entries_file(L, siren):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert L.load().inr_forward(siren, None, p, p, p, 1, p, None, None) != 0
    assert L.last_error() == "inr_forward: null argument"


def test_offgrid_entries_file(L):
    n = C.c_int64(-1)
    assert L.load().inr_nudft_scratch(2, 8, 8, 0, C.byref(n)) != 0
    assert L.last_error() == "inr_nudft_scratch: M = 0 (1 <= M < 2^31 samples per call)"
    assert n.value == -1


def test_other_entries_file_and_one_text_per_thread(L):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert L.load().inr_encode_gauss(p, p, 0, 8, p, None) != 0  # (refused before any launch)
    assert L.last_error() == "inr_encode_gauss: B = 0, E = 8"
    seen = []

    def other():
        text = C.create_string_buffer(512)
        seen.append((L.load().inr_last_error(text, 512), text.value))

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == [(0, b"")]
    assert L.last_error() == "inr_encode_gauss: B = 0, E = 8"  # ... and this thread still has its own
