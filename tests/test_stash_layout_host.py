"""The fp32 activation-stash layout (csrc/inr_stash.h) on the host: tools/probes/stash_layout_check.cpp includes nothing but
that header, is built here with the host C++ compiler and checks, over a grid of shapes, that the pieces of a tile's stash
are 16-byte aligned, pairwise disjoint and tile [0, floats_per_tile) exactly.  It also prints floats_per_tile for the fp32
plan descriptions that tests/golden/host_layout.json pins (those of tests/test_host.py among them); they are held against
save_bytes_per_tile of the built library (CPU only: creating and sizing a plan touches no GPU)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import layout_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "probes", "stash_layout_check.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "host_layout.json")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def _shape_line(L, d, tile_rows, blocks):
    """a plan description as the probe takes it: the shape the header is asked about, from the description and from what
    the library says about its tiles (rows per tile, hidden row blocks)"""
    k_rows = 32 * ((d["in_features"] + 31) // 32)  # rows of the input-feature image: whole 32-row k-blocks
    if d["kind"] in (L.KIND_FOURIER, L.KIND_MSFOURIER, L.KIND_MSBOUNDED, L.KIND_GABOR, L.KIND_KGABOR):
        n = d["depth"]  # live stages: up to the last head (multiscale heads sit behind stages 1, 3, 5, 7)
        last = max(s for s in (1, 3, 5, 7) if s <= n) if d["kind"] in (L.KIND_MSFOURIER, L.KIND_MSBOUNDED) else n
        return "mfn %d %d %d %d" % (blocks, tile_rows, last + 1, k_rows)
    wire = d["kind"] in (L.KIND_WIRE, L.KIND_WIRE2D)
    ns = 7 if d["kind"] == L.KIND_WIRE2D else (3 if wire else 2)
    depth = d["depth"] + 2 if wire else d["depth"]  # WIRE counts its hidden complex layers only
    return "mlp %d %d %d %d %d" % (blocks, tile_rows, ns, depth, k_rows if d["input"] == L.INPUT_GAUSS else 0)


def test_stash_layout_check(tmp_path):
    from inr_mi355x import _lib as L
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler (c++, g++, clang++ or $CXX)"
    exe = str(tmp_path / "stash_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)

    with open(GOLD) as f:
        plans = T.unpack(json.load(f))
    lib = L.load()
    lines, want = [], []
    for p in plans:
        d = p["desc"]
        if p["create"][0] != 0 or p["one_class"] or d["precision"] != L.PRECISION_F32:
            continue
        plan, sz, info = C.c_void_p(), L.Sizes(), L.StepInfo()
        assert lib.inr_plan_create(C.byref(L.NetDesc(**d)), C.byref(plan)) == 0, L.last_error()
        assert lib.inr_plan_sizes(plan, C.byref(sz)) == 0, L.last_error()
        assert lib.inr_plan_step_info(plan, 100, C.byref(info)) == 0, L.last_error()
        lib.inr_plan_destroy(plan)
        assert sz.save_bytes_per_tile == p["sizes"][1 + T.SIZES_FIELDS.index("save_bytes_per_tile")], d
        lines.append(_shape_line(L, d, sz.tile_rows, info.hidden_blocks))
        want.append(sz.save_bytes_per_tile // 4)
    kinds = {p["desc"]["kind"] for p in plans if p["create"][0] == 0}
    assert len(lines) >= 100 and kinds >= {L.KIND_SIREN, L.KIND_FFN, L.KIND_WIRE, L.KIND_WIRE2D, L.KIND_FOURIER,
                                           L.KIND_MSFOURIER, L.KIND_MSBOUNDED, L.KIND_GABOR}
    shapes = tmp_path / "shapes.txt"
    shapes.write_text("\n".join(lines) + "\n")

    run = subprocess.run([exe, str(shapes)], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr)
    assert run.returncode == 0, run.stdout
    assert "grid cases: ok" in run.stdout
    got = [int(l.split()[1]) for l in run.stdout.splitlines() if l.startswith("floats_per_tile ")]
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        assert g == w, (line, g, w)
