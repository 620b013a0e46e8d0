"""The host layout table: what the built library answers, on a CPU, for plan x batch size x environment switches.
tools/make_golden.py (part ``host_layout``) records it from one commit's library into tests/golden/host_layout.json;
tests/test_layout_host.py replays it against the library under test.  A plain module, like matrix_cases.py, so that the
recorder and the test ask the library in the same words."""
from __future__ import annotations

import ctypes as C
import os

B_VALUES = [0, 1, 100, 129, 4133, 19200, 25000, 38400, 65536, 100000, 235520, 3532800]
SWITCHES = [(rs, ov) for rs in (None, "0", "1") for ov in (None, "0")]  # (INR_RS, INR_OVERLAP)
DESC_FIELDS = ["kind", "in_features", "width", "depth", "out_features", "last_act", "input", "enc_size", "w0",
               "first_omega_0", "hidden_omega_0", "scale_0", "precision"]
SIZES_FIELDS = ["n_params", "packed_floats", "tile_rows", "save_bytes_per_tile", "max_blocks", "slab_floats",
                "step_save_by_tile"]
INFO_FIELDS = ["row_split", "ncb", "grid", "rounds", "hi", "lo", "n_hi", "hidden_blocks"]
_ENV = ("INR_RS", "INR_OVERLAP", "INR_GEMM_ONE_CLASS", "INR_GEMM_ENC_COST")


def plan_record(L, kw: dict, one_class: bool) -> dict:
    """One plan's part of the table: creation (with INR_GEMM_ONE_CLASS set or not), sizes and, per batch size, launch
    dims + per switch setting (workspace, step info).  A call is [rc, values...], a failed one [rc, message].  Where
    the six switch settings of a batch size agree, one entry stands for all.  The environment is left as found."""
    lib = L.load()
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    rec = {"desc": kw, "one_class": one_class}
    try:
        if one_class:
            os.environ["INR_GEMM_ONE_CLASS"] = "1"
        plan = C.c_void_p()
        rc = lib.inr_plan_create(C.byref(L.NetDesc(**kw)), C.byref(plan))
        os.environ.pop("INR_GEMM_ONE_CLASS", None)  # (read at creation only)
        rec["create"] = [rc] if rc == 0 else [rc, L.last_error()]
        if rc != 0:
            return rec
        sz = L.Sizes()
        rc = lib.inr_plan_sizes(plan, C.byref(sz))
        rec["sizes"] = [rc] + [int(getattr(sz, f)) for f in SIZES_FIELDS]
        rec["rows"] = []
        for B in B_VALUES:
            a, b = C.c_int64(), C.c_int64()
            rc = lib.inr_plan_launch_dims(plan, B, C.byref(a), C.byref(b))
            row = {"dims": [rc, a.value, b.value] if rc == 0 else [rc, L.last_error()], "sw": []}
            for rs, ov in SWITCHES:
                for k, v in (("INR_RS", rs), ("INR_OVERLAP", ov)):
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
                rc = lib.inr_plan_workspace(plan, B, C.byref(a), C.byref(b))
                ws = [rc, a.value, b.value] if rc == 0 else [rc, L.last_error()]
                info = L.StepInfo()
                rc = lib.inr_plan_step_info(plan, B, C.byref(info))
                si = [rc] + [int(getattr(info, f)) for f in INFO_FIELDS] if rc == 0 else [rc, L.last_error()]
                row["sw"].append([ws, si])
            if all(s == row["sw"][0] for s in row["sw"]):
                row["sw"] = row["sw"][:1]
            rec["rows"].append(row)
        lib.inr_plan_destroy(plan)
        return rec
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def plans(L) -> list:
    """The plan descriptions of the table, [(NetDesc keywords, INR_GEMM_ONE_CLASS set at creation)]: every description of
    the conformance matrix, those of tests/test_host.py (refused ones too: code and message are part of the record), bf16
    SIREN at depths 3 / 5 / 8, WIRE at 12 blocks, WIRE2D at 16, the 512-wide multiscale filter network on both inputs,
    and the shapes of tests/test_gpu_workspace_exact.py.  Only the recorder calls this (it builds the matrix's models)."""
    import matrix_cases as MC
    descs = []

    def add(**kw):
        kw = {f: kw.get(f, 0) for f in DESC_FIELDS}
        if kw not in descs:
            descs.append(kw)

    seen = set()
    for c in sorted(MC.CASES, key=lambda c: c.loss != "L2"):  # (an L2 case of a description needs no oracle forward)
        key = (c.family, c.build, c.width, c.depth, c.size, c.input, c.out_f, c.last)
        if key in seen:
            continue
        seen.add(key)
        d = MC.prepare(c).engine.desc
        add(**{f: getattr(d, f) for f in DESC_FIELDS})
    siren = dict(kind=L.KIND_SIREN, in_features=512, width=256, depth=5, out_features=2, last_act=L.ACT_TANH,
                 input=L.INPUT_GAUSS, enc_size=256, w0=30.0)
    add(**siren)
    add(kind=L.KIND_SIREN, in_features=16, width=32, depth=4, out_features=2, last_act=L.ACT_TANH, input=L.INPUT_GAUSS,
        enc_size=8, w0=30.0)
    for bad in (dict(width=513), dict(width=0), dict(depth=1), dict(out_features=9), dict(in_features=500), dict(kind=99)):
        add(**dict(siren, **bad))
    for bad in (dict(width=512), dict(width=64), dict(depth=9), dict(enc_size=40, in_features=80), dict(input=L.INPUT_X)):
        add(**dict(siren, precision=L.PRECISION_BF16, **bad))
    for in_f in (3, 16, 42, 512):
        for kind in (L.KIND_FOURIER, L.KIND_GABOR, L.KIND_MSBOUNDED):
            add(kind=kind, in_features=in_f, width=48, depth=3, out_features=2, input=L.INPUT_X)
    add(kind=L.KIND_FOURIER, in_features=500, width=48, depth=3, out_features=2, input=L.INPUT_GAUSS, enc_size=256)
    for depth in (3, 5, 8):
        add(**dict(siren, depth=depth, precision=L.PRECISION_BF16))
    add(kind=L.KIND_WIRE, in_features=3, width=181, depth=2, out_features=2, input=L.INPUT_X, first_omega_0=30.0,
        hidden_omega_0=30.0, scale_0=15.0)
    add(kind=L.KIND_WIRE2D, in_features=3, width=256, depth=2, out_features=2, input=L.INPUT_X, first_omega_0=20.0,
        hidden_omega_0=20.0, scale_0=10.0)
    for depth in (1, 8):
        add(kind=L.KIND_MSFOURIER, in_features=512, width=512, depth=depth, out_features=2, input=L.INPUT_GAUSS, enc_size=256)
        add(kind=L.KIND_MSFOURIER, in_features=512, width=512, depth=depth, out_features=2, input=L.INPUT_X)
    # tests/test_gpu_workspace_exact.py: depth 3 behind a gauss encoder of 32
    small = dict(siren, depth=3, in_features=64, enc_size=32, last_act=L.ACT_ID)
    for extra in (dict(width=32), dict(), dict(precision=L.PRECISION_BF16)):
        add(**dict(small, **extra))
    add(kind=L.KIND_MSFOURIER, in_features=64, width=512, depth=1, out_features=2, input=L.INPUT_GAUSS, enc_size=32)
    return [(d, False) for d in descs] + [(d, True) for d in descs if d["precision"] == L.PRECISION_BF16]


def pack(records: list) -> dict:
    """the recorded plans as they are written to the file: descriptions as value lists (DESC_FIELDS order), and the rows
    of plans that answer alike (same build, another output size, ...) stored once, in ``row_sets``"""
    sets, plans = [], []
    for r in records:
        r = dict(r, desc=[r["desc"][f] for f in DESC_FIELDS])
        if "rows" in r:
            if r["rows"] not in sets:
                sets.append(r["rows"])
            r["rows"] = sets.index(r["rows"])
        plans.append(r)
    return {"row_sets": sets, "plans": plans}


def unpack(table: dict) -> list:
    out = []
    for r in table["plans"]:
        r = dict(r, desc=dict(zip(DESC_FIELDS, r["desc"])))
        if "rows" in r:
            r["rows"] = table["row_sets"][r["rows"]]
        out.append(r)
    return out


def dump(table: dict, path: str) -> None:
    """one plan / one row set per line"""
    import json
    enc = lambda o: json.dumps(o, separators=(",", ":"))
    head = {k: v for k, v in table.items() if k not in ("row_sets", "plans")}
    with open(path, "w") as f:
        f.write("{" + enc(head)[1:-1] + ',\n"row_sets":[\n' + ",\n".join(enc(r) for r in table["row_sets"]))
        f.write('\n],\n"plans":[\n' + ",\n".join(enc(r) for r in table["plans"]) + "\n]}\n")
