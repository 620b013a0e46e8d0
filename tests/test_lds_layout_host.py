"""The kernels' dynamic-LDS layouts (csrc/inr_lds.h) on the host: tools/probes/lds_layout_check.cpp includes nothing but that
header, is built here with the host C++ compiler and checks, over every instantiated shape and a grid of encoder sizes, that
the pieces of a block are disjoint, aligned where the kernel needs it and end at the launch size.  The launch sizes it
prints are held against tests/golden/lds_layout.json, the byte counts of the launchers' formulas before the header existed;
the narrow MLP's option thresholds against the sizes tests/test_gpu_lds_options.py runs at.  The last test drives a launch
that cannot fit through the built library: the launcher refuses it on the host (CPU only: no HIP call precedes the size
comparison), and the library goes on answering."""
import ctypes as C
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "probes", "lds_layout_check.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "lds_layout.json")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_lds_layout_check(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler (c++, g++, clang++ or $CXX)"
    exe = str(tmp_path / "lds_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr)
    assert run.returncode == 0, run.stdout
    assert "lds layouts: ok" in run.stdout

    with open(GOLD) as f:
        want = json.load(f)
    got = {}
    for line in run.stdout.splitlines():
        if line.startswith("bytes "):
            key, n = line[len("bytes "):].rsplit(" : ", 1)
            got[key] = int(n)
    # a launch of the row-split kernel reserves the partial outputs of 4 rows: the smaller ones are checked, not launched
    launched = {k: v for k, v in got.items() if not (k.startswith("rs ") and not k.endswith(" mo 4"))}
    assert len(want) >= 190 and sorted(launched) == sorted(want)
    for key, n in want.items():
        assert launched[key] == n, (key, launched[key], n)

    thr = {}
    for line in run.stdout.splitlines():
        if line.startswith("threshold mlp "):
            key, vals = line[len("threshold mlp "):].split(" : ")
            v = vals.split()
            thr[key] = dict(zip(v[0::2], map(int, v[1::2])))
    assert sorted(thr) == ["nb %d nw 4 ld 36" % nb for nb in (1, 2, 4, 8)]
    # 147 456 B of images leave 16 384 B: 12 B per encoder row, 4 112 B of fragments, 4 608 B of dZ_last images
    assert thr["nb 8 nw 4 ld 36"] == dict(dz_off=640, ll_off=1024, base_off=1368)
    for t in thr.values():
        assert 0 < t["dz_off"] < t["ll_off"] < t["base_off"]


def test_an_oversize_launch_is_refused_on_the_host():
    from inr_mi355x import _lib as L
    lib = L.load()

    def plan_of(E):
        d = L.NetDesc(kind=L.KIND_SIREN, in_features=2 * E, width=256, depth=3, out_features=2, last_act=L.ACT_ID,
                      input=L.INPUT_GAUSS, enc_size=E, w0=30.0, precision=L.PRECISION_F32)
        plan = C.c_void_p()
        assert lib.inr_plan_create(C.byref(d), C.byref(plan)) == 0, L.last_error()
        return plan

    big = plan_of(1368)  # the first enc_size whose images + encoder matrix exceed the CU (the probe's base_off)
    buf = (C.c_float * 16)()  # stands for every device buffer: the refusal comes before anything could read one
    p = C.cast(buf, C.c_void_p)
    rc = lib.inr_forward(big, p, p, p, p, 401, p, None, None)
    assert rc not in (0, L.ERR_UNSUPPORTED) and "inr mlp kernel launch" in L.last_error(), (rc, L.last_error())
    lib.inr_plan_destroy(big)
    ok, nt, nb = plan_of(256), C.c_int64(), C.c_int64()
    assert lib.inr_plan_launch_dims(ok, 401, C.byref(nt), C.byref(nb)) == 0, L.last_error()
    assert (nt.value, nb.value) == (4, 4)
    lib.inr_plan_destroy(ok)
