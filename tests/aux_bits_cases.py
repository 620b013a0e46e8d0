"""Cases of tests/test_gpu_aux_bits.py and of tools/make_golden.py's part ``aux_bits``: every helper kernel of the engine
(slab reduction, Adam + re-pack, penalty gradients, losses, encoders, shuffle, and the metric / display / band / coil
kernels that share the block reduction of csrc/inr_reduce.h) on the smallest shapes at which each of its paths can go
wrong, through the public entries only.  A case returns {buffer name: SHA-256 of its bytes}; tests/golden/aux_bits.json
holds what one named commit's library gave.  All of these kernels sum in a fixed order: the bits are the contract.

Inputs come from a closed formula (an integer hash of the element index, mapped to fp32), never from a torch generator.
``python tests/aux_bits_cases.py`` prints the table of the library that INR_LIB_PATH names as JSON."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

BOUNDS4 = [(0.0, 0.2), (0.0, 0.45), (0.0, 0.8), (0.0, 5.0)]
# Slab counts of the fused kernel's set (the chunk-slab sets of the weight-gradient GEMM have whatever the layout gives
# that batch): one; a short tail only; and the first count >= 33 that is odd, 5 or more past a multiple of 16 and leaves
# the last wave's quarter of the flat sum 9 or more -- the 8-deep batch plus a tail in EVERY wave's quarter, the 16-deep
# batch plus the long tail form of slab_sum (3 takes the short form).  "third_set" (bf16 plan only): 50 tiles, where the
# first layer's GEMM units get a chunk count of their own (SlabSplit.n3 > 0).
SLAB_TARGETS = ("1", "3", "33+")
THIRD_SET_TILES = 50


def rnd(n, seed, scale=1.0):
    """n fp32 values in [-scale, scale): 24 bits of a 32-bit hash of (index, seed); every step is exact"""
    u = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32((seed * 40503 + 12345) & 0xFFFFFFFF)
    u ^= u >> np.uint32(15)
    u *= np.uint32(2246822519)
    u ^= u >> np.uint32(13)
    u *= np.uint32(3266489917)
    u ^= u >> np.uint32(16)
    return (((u >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23)) - np.float32(1.0)) * np.float32(scale)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from inr_mi355x import _lib as L
    return L, L.load()


# ---- slab reduction + Adam + pack -----------------------------------------------------------------------------------
def _engine(plan):
    from inr_mi355x import _lib as L
    from inr_mi355x.engine import MLPEngine, MFNEngine
    if plan in ("siren32", "siren32_by_image"):  # flat slab layout: fused reduce + Adam
        return MLPEngine(L.KIND_SIREN, 16, 32, 4, 2, L.ACT_ID, L.INPUT_GAUSS, 8, 30.0)
    if plan == "siren256":  # weight-gradient GEMM: a second slab set
        return MLPEngine(L.KIND_SIREN, 512, 256, 5, 2, L.ACT_ID, L.INPUT_GAUSS, 256, 30.0)
    if plan == "siren256_bf16":  # ... and a third
        return MLPEngine(L.KIND_SIREN, 512, 256, 5, 2, L.ACT_ID, L.INPUT_GAUSS, 256, 30.0, precision=L.PRECISION_BF16)
    if plan == "wire":  # generic reduction, complex entries
        return MLPEngine(L.KIND_WIRE, 3, 32, 2, 2, L.ACT_ID, L.INPUT_X, 0, 0.0, 10.0, 10.0, 5.0)
    if plan == "wire2d":
        return MLPEngine(L.KIND_WIRE2D, 3, 32, 2, 2, L.ACT_ID, L.INPUT_X, 0, 0.0, 10.0, 10.0, 5.0)
    if plan == "gabor":  # filter network with centres: gabor_finish, gabor_m2
        return MFNEngine(L.KIND_GABOR, 16, 32, 3, 2, 8)
    raise KeyError(plan)


STEP_PLANS = ("siren32", "siren256", "siren256_bf16", "wire", "wire2d", "gabor", "siren32_by_image")


def _batch_for(eng, target):
    """smallest B = k * tile_rows - 1 whose slab count (inr_plan_launch_dims) is the target"""
    if target == "third_set":
        B = THIRD_SET_TILES * eng.tile_rows - 1
        nb, chunk_slabs = eng.launch_dims(B)[1], eng.workspace(B)[1] - eng.launch_dims(B)[1]
        # one class of GEMM units would have at most 256 / 6 units = 42 chunks each: more chunk slabs than that means the
        # first layer's units are chunked on their own, i.e. the reduction reads a third slab count
        if chunk_slabs <= 256 // 6:
            raise RuntimeError(f"{chunk_slabs} chunk slabs at B = {B}: no third slab set")
        return B, nb
    for k in range(1, 400):
        B = max(k * eng.tile_rows - 1, 1)
        nb = eng.launch_dims(B)[1]
        big = nb >= 33 and nb % 2 == 1 and nb % 16 > 4 and nb - 3 * ((nb + 3) // 4) >= 9
        if (target == "33+" and big) or (target != "33+" and nb == int(target)):
            return B, nb
    raise RuntimeError(f"no batch size gives {target} slabs")


def step_case(plan, target):
    from inr_mi355x import _lib as L
    from inr_mi355x.engine import LossSpec, MFNEngine
    old = os.environ.get("INR_PACK_BY_IMAGE")
    if plan == "siren32_by_image":
        os.environ["INR_PACK_BY_IMAGE"] = "1"
    try:
        eng = _engine(plan)
        B, nb = _batch_for(eng, target)
        p0 = dev(rnd(eng.n_params, 1, 0.1))
        eng.bind(p0.clone())
        out = {"B": str(B), "slabs": str(nb), "all_slabs": str(eng.workspace(B)[1]),
               "pack/packed": sha(eng.packed)}  # inr_pack_params
        gauss = eng.input_mode == L.INPUT_GAUSS
        x = dev(rnd(B * 3, 2).reshape(B, 3))
        enc_B = dev(rnd(eng.in_features // 2 * 3, 3, 2.0).reshape(-1, 3)) if gauss else None
        gt = dev(rnd(B * 2, 4, 0.3).reshape(B, 2))
        spec = LossSpec(L.LOSS_L2_HALF, 1e-3, 2.0, 0.5, 3000)
        real = plan.startswith("siren")
        kw = dict(weight_decay=1e-4, l1=1e-6 if real else 0.0, l2=1e-5 if real else 0.0)
        modes = ("two_calls", "dev") if isinstance(eng, MFNEngine) else ("two_calls", "one_call", "dev")
        sched = np.empty(8, dtype=np.float32)
        L.check(eng.lib.inr_adam_schedule(1e-3, 0.9, 0.999, 4, sched.ctypes.data))
        sched_dev = dev(sched)
        for mode in modes:
            eng.params.copy_(p0)
            eng.exp_avg.zero_()
            eng.exp_avg_sq.zero_()
            eng.step = 0
            eng.pack()
            step_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
            for s in (1, 2):
                if mode == "one_call":
                    eng.train_adam_step(x, enc_B, gt, spec, 1e-3, **kw)
                else:
                    eng.train_step(x, enc_B, gt, spec)
                    if mode == "two_calls":
                        eng.adam_step(1e-3, **kw)
                    else:  # inr_adam_step_dev with a 4-entry schedule
                        L.check(eng.lib.inr_adam_step_dev(eng.plan, eng.params.data_ptr(), eng.grads.data_ptr(),
                                                          eng.exp_avg.data_ptr(), eng.exp_avg_sq.data_ptr(),
                                                          eng.packed.data_ptr(), sched_dev.data_ptr(), 4,
                                                          step_dev.data_ptr(), 0.9, 0.999, 1e-8, kw["weight_decay"],
                                                          kw["l1"], kw["l2"], _stream()))
                for name, t in (("grads", eng.grads), ("loss", eng._loss_word), ("params", eng.params),
                                ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq), ("packed", eng.packed)):
                    out[f"{mode}/step{s}/{name}"] = sha(t)
        return out
    finally:
        if old is None:
            os.environ.pop("INR_PACK_BY_IMAGE", None)
        else:
            os.environ["INR_PACK_BY_IMAGE"] = old


def shard_case():
    """inr_adam_step_shard on [0, P), [1, P - 1) and the empty [5, 5)"""
    from inr_mi355x import _lib as L
    eng = _engine("siren32")
    P = eng.n_params
    p0 = dev(rnd(P, 1, 0.1))
    eng.bind(p0.clone())
    g = dev(rnd(P, 5, 1e-2))
    out = {}
    for lo, hi in ((0, P), (1, P - 1), (5, 5)):
        eng.params.copy_(p0)
        eng.exp_avg.zero_()
        eng.exp_avg_sq.zero_()
        for step in (1, 2):
            L.check(eng.lib.inr_adam_step_shard(eng.plan, eng.params.data_ptr(), g[lo:].data_ptr(), eng.exp_avg.data_ptr(),
                                                eng.exp_avg_sq.data_ptr(), lo, hi, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1e-6, 1e-5,
                                                step, _stream()))
        for name, t in (("params", eng.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
            out[f"{lo}_{hi}/{name}"] = sha(t)
    return out


def reg_case(plan):
    """inr_reg_grad: l1, l2 and both; on WIRE with an l2_dir, and with [lo, hi) cutting a complex pair in two"""
    eng = _engine(plan)
    P = eng.n_params
    eng.bind(dev(rnd(P, 1, 0.1)))
    l2_dir = dev(np.array([0.6, -0.8], dtype=np.float32)) if plan == "wire" else None
    ranges = [(0, P)] + ([(P - 7, P - 2), (P - 6, P - 1)] if plan == "wire" else [(3, P - 5)])  # odd and even cuts
    out = {}
    for lo, hi in ranges:
        for tag, l1, l2 in (("l1", 1e-3, 0.0), ("l2", 0.0, 1e-2), ("both", 1e-3, 1e-2)):
            g = dev(rnd(hi - lo, 6, 1e-2))
            eng.reg_grad(l1, l2, l2_dir, grads=g, lo=lo, hi=hi)
            out[f"{lo - P}_{hi - P}/{tag}"] = sha(g)
    return out


# ---- losses ---------------------------------------------------------------------------------------------------------
def _loss_desc(kind, count):
    from inr_mi355x import _lib as L
    return L.LossDesc(kind=kind, eps=1e-3, sigma=2.0, factor=0.5, inv_count=1.0 / count, hdr_A=0.37)


def _mask(B, seed):
    return dev((rnd(B, seed) > -0.2).astype(np.uint8))


def loss_case(B):
    """every loss kind, with and without a mask; B = 1: 63 empty blocks, 16449: a lane visits two rows"""
    L, lib = _lib()
    out_ = dev(np.abs(rnd(B * 2, 7, 0.3)).reshape(B, 2) + np.float32(0.05))  # positive: MSLE takes logarithms
    sgn = dev(rnd(B * 2, 8, 0.3).reshape(B, 2))
    gt = dev(np.abs(rnd(B * 2, 9, 0.3)).reshape(B, 2) + np.float32(0.05))
    mask = _mask(B, 10)
    res = {}
    for kind in range(L.LOSS_L2_HALF, L.LOSS_CENTER + 1):
        y = out_ if kind == L.LOSS_MSLE_HALF else sgn
        for tag, m in (("all", None), ("mask", mask)):
            loss = torch.zeros(L.LOSS_WORDS, device="cuda")
            dout = torch.full_like(y, float("nan"))
            ld = _loss_desc(kind, B)
            L.check(lib.inr_loss_grad(C.byref(ld), y.data_ptr(), gt.data_ptr(), None, None if m is None else m.data_ptr(), B,
                                      loss.data_ptr(), dout.data_ptr(), _stream()))
            res[f"kind{kind}/{tag}/loss"] = sha(loss)
            res[f"kind{kind}/{tag}/dout"] = sha(dout)
    return res


def loss_multi_case():
    L, lib = _lib()
    B = 257
    gt = dev(rnd(B * 2, 9, 0.3).reshape(B, 2))
    dist = dev(np.abs(rnd(B, 11, 1.0)))
    mask = _mask(B, 10)
    res = {}
    for NH in (1, 4):
        outs = dev(rnd(NH * B * 2, 12, 0.3).reshape(NH, B, 2))
        for tag, cons in (("plain", False), ("cons", True)):
            for kind in (L.LOSS_L2_HALF, L.LOSS_LOGSPACE):
                ld = _loss_desc(kind, B)
                ld.scale = 0.5
                if cons:
                    ld.cons_w, ld.cons_chan = 0.1, 2
                    for i, (lo, hi) in enumerate(BOUNDS4):
                        ld.cons_lo[i], ld.cons_hi[i], ld.cons_inv[i] = lo, hi, 1.0 / (2 * B)
                loss = torch.zeros(L.LOSS_WORDS, device="cuda")
                douts = torch.full_like(outs, float("nan"))
                L.check(lib.inr_loss_grad_multi(C.byref(ld), outs.data_ptr(), gt.data_ptr(), dist.data_ptr() if cons else None,
                                                mask.data_ptr(), NH, B, loss.data_ptr(), douts.data_ptr(), _stream()))
                res[f"heads{NH}/{tag}/kind{kind}/loss"] = sha(loss)
                res[f"heads{NH}/{tag}/kind{kind}/douts"] = sha(douts)
    return res


def tv_case(R, R_own, W, H, pointwise_only=False):
    """inr_tv_grad (adds into loss and dout) and inr_loss_tv_grad (writes them) on R rows of width W"""
    L, lib = _lib()
    n = R * W
    y = dev(rnd(n * 2, 13, 0.3).reshape(n, 2))
    gt = dev(rnd(n * 2, 14, 0.3).reshape(n, 2))
    mask = _mask(n, 15)
    res = {}
    if not pointwise_only:
        loss = torch.zeros(L.LOSS_WORDS, device="cuda")
        loss[0] = 0.25
        dout = dev(rnd(n * 2, 16, 0.1).reshape(n, 2))
        L.check(lib.inr_tv_grad(y.data_ptr(), R, R_own, W, H, C.c_float(1e-4), loss.data_ptr(), dout.data_ptr(), _stream()))
        res["tv/loss"], res["tv/dout"] = sha(loss), sha(dout)
    for tag, m in (("all", None), ("mask", mask)):
        loss = torch.zeros(L.LOSS_WORDS, device="cuda")
        dout = torch.full_like(y, float("nan"))
        ld = _loss_desc(L.LOSS_L2_HALF, n)
        L.check(lib.inr_loss_tv_grad(C.byref(ld), y.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(), R, R_own,
                                     W, H, C.c_float(1e-4), loss.data_ptr(), dout.data_ptr(), _stream()))
        res[f"loss_tv/{tag}/loss"], res[f"loss_tv/{tag}/dout"] = sha(loss), sha(dout)
    return res


def center_case():
    """n = 1, and n = 300 with three indices outside [0, B); a rows distinct, b rows distinct, no row in both"""
    L, lib = _lib()
    B = 700
    y = dev(rnd(B * 2, 17, 0.3).reshape(B, 2))
    gt = dev(rnd(B * 2, 18, 0.3).reshape(B, 2))
    i = np.arange(300, dtype=np.int64)
    ia, ib = (i * 11) % 350, 350 + (i * 13) % 350
    ia[5], ib[17], ia[100] = -1, B, 10 ** 9
    res = {}
    for n in (1, 300):
        loss = torch.zeros(L.LOSS_WORDS, device="cuda")
        loss[0] = 0.25
        dout = dev(rnd(B * 2, 19, 0.1).reshape(B, 2))
        a, b = dev(ia[:n].copy()), dev(ib[:n].copy())
        L.check(lib.inr_center_pairs_grad(y.data_ptr(), gt.data_ptr(), a.data_ptr(), b.data_ptr(), n, B, C.c_float(0.1 / n),
                                          loss.data_ptr(), dout.data_ptr(), _stream()))
        res[f"n{n}/loss"], res[f"n{n}/dout"] = sha(loss), sha(dout)
    return res


# ---- encoders, shuffle ----------------------------------------------------------------------------------------------
def encode_case():
    from inr_mi355x.engine import encode_gauss, encode_logf
    coords = dev(rnd(300 * 3, 20).reshape(300, 3))
    return {"gauss": sha(encode_gauss(coords, dev(rnd(8 * 3, 21, 2.0).reshape(8, 3)))),
            "logf": sha(encode_logf(coords, dev(np.array([1.0, 2.5, 6.25], dtype=np.float32))))}


def shuffle_case(n):
    """all four row arrays, order_out and batch_counts (a batch size that does not divide n), two epochs"""
    L, lib = _lib()
    bs = max(n // 3 - 1, 1) if n > 1 else 1
    nb = (n + bs - 1) // bs
    coords, gt = dev(rnd(n * 3, 22).reshape(n, 3)), dev(rnd(n * 2, 23).reshape(n, 2))
    dist, mask = dev(rnd(n, 24)), _mask(n, 25)
    res = {}
    for epoch in (0, 1):
        co, go, do, mo = (torch.zeros_like(t) for t in (coords, gt, dist, mask))
        counts = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        order = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        L.check(lib.inr_shuffle_epoch(n, bs, C.c_uint64(0x123456789ABCDEF), epoch, coords.data_ptr(), gt.data_ptr(),
                                      dist.data_ptr(), mask.data_ptr(), co.data_ptr(), go.data_ptr(), do.data_ptr(),
                                      mo.data_ptr(), counts.data_ptr(), order.data_ptr(), _stream()))
        for name, t in (("coords", co), ("gt", go), ("dist", do), ("mask", mo), ("counts", counts), ("order", order)):
            res[f"epoch{epoch}/{name}"] = sha(t)
    return res


# ---- helpers whose tree moved into the shared header ----------------------------------------------------------------
def metrics_case(H, W):
    L, lib = _lib()
    Cn = 2
    coils = dev(rnd(Cn * H * W * 2, 26, 0.5).reshape(Cn, H, W, 2))
    ref = dev(np.abs(rnd(H * W, 27, 0.7)).reshape(H, W))
    n = C.c_int64()
    L.check(lib.inr_image_metrics_scratch(Cn, H, W, C.byref(n)))
    scratch = torch.zeros(n.value, dtype=torch.float64, device="cuda")
    rss = torch.zeros(H, W, device="cuda")
    metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.float64, device="cuda")
    L.check(lib.inr_image_metrics(coils.data_ptr(), Cn, H, W, ref.data_ptr(), rss.data_ptr(), metrics.data_ptr(),
                                  scratch.data_ptr(), n.value, _stream()))
    return {"rss": sha(rss), "metrics": sha(metrics)}


def display_case():
    L, lib = _lib()
    Cn, H, W = 2, 9, 11
    coils = dev(rnd(Cn * H * W * 2, 28, 0.5).reshape(Cn, H, W, 2))
    minus = dev(rnd(Cn * H * W * 2, 29, 0.5).reshape(Cn, H, W, 2))
    res = {}
    n = C.c_int64()
    L.check(lib.inr_kspace_display_scratch(Cn, H, W, C.byref(n)))
    for tag, m in (("plain", None), ("minus", minus)):
        scratch = torch.zeros(n.value, device="cuda")
        pic = torch.zeros(H, W, device="cuda")
        L.check(lib.inr_kspace_display(coils.data_ptr(), None if m is None else m.data_ptr(), Cn, H, W, C.c_float(5.0),
                                       pic.data_ptr(), scratch.data_ptr(), n.value, _stream()))
        res[f"kspace_display/{tag}"] = sha(pic)
    img = dev(rnd(H * W, 30, 3.0).reshape(H, W))
    lut = dev(((np.arange(256) * 7 + 3) % 256).astype(np.uint8))
    L.check(lib.inr_gray8_scratch(H, W, C.byref(n)))
    for tag, has_range in (("own_range", 0), ("given_range", 1)):
        scratch = torch.zeros(n.value, device="cuda")
        out = torch.zeros(H, W, dtype=torch.uint8, device="cuda")
        norm = torch.zeros(H, W, device="cuda")
        L.check(lib.inr_gray8(img.data_ptr(), H, W, 1, has_range, C.c_float(0.25), C.c_float(2.0), lut.data_ptr(),
                              out.data_ptr(), norm.data_ptr(), scratch.data_ptr(), n.value, _stream()))
        res[f"gray8/{tag}/bytes"], res[f"gray8/{tag}/norm"] = sha(out), sha(norm)
    L.check(lib.inr_coil_stats_scratch(Cn, H, W, C.byref(n)))
    scratch = torch.zeros(n.value, dtype=torch.float64, device="cuda")
    stats = torch.zeros(Cn, 4, dtype=torch.float64, device="cuda")
    L.check(lib.inr_coil_stats(coils.data_ptr(), Cn, H, W, stats.data_ptr(), scratch.data_ptr(), n.value, _stream()))
    res["coil_stats"] = sha(stats)
    return res


def bands_case():
    L, lib = _lib()
    n, K = 1025, 3
    dist, mask = dev(np.abs(rnd(n, 31, 1.4))), _mask(n, 34)
    gt, pred = dev(rnd(n * 2, 32, 0.5).reshape(n, 2)), dev(rnd(n * 2, 33, 0.5).reshape(n, 2))
    lo, hi = (C.c_float * K)(0.0, 0.3, 0.2), (C.c_float * K)(0.3, 0.9, 5.0)
    ns = C.c_int64()
    L.check(lib.inr_band_stats_scratch(n, K, C.byref(ns)))
    res = {}
    for tag, p, m in (("pred", pred, None), ("gt_only_masked", None, mask)):
        scratch = torch.zeros(ns.value, dtype=torch.float64, device="cuda")
        stats = torch.zeros(K, L.BAND_FIELDS, dtype=torch.float64, device="cuda")
        L.check(lib.inr_band_stats(dist.data_ptr(), gt.data_ptr(), None if p is None else p.data_ptr(),
                                   None if m is None else m.data_ptr(), 1, n, lo, hi, K, stats.data_ptr(),
                                   scratch.data_ptr(), _stream()))
        res[tag] = sha(stats)
    return res


def coil_gram_case():
    L, lib = _lib()
    Cn, N = 3, 129
    x = dev(rnd(Cn * N * 2, 35, 0.5).reshape(Cn, N, 2))
    ns = C.c_int64()
    L.check(lib.inr_coil_gram_scratch(Cn, N, C.byref(ns)))
    scratch = torch.zeros(ns.value, dtype=torch.float64, device="cuda")
    gram = torch.zeros(Cn, Cn, 2, dtype=torch.float64, device="cuda")
    L.check(lib.inr_coil_gram(x.data_ptr(), Cn, N, gram.data_ptr(), scratch.data_ptr(), ns.value, _stream()))
    return {"gram": sha(gram)}


CASES = {f"step/{p}/slabs{t}": (lambda p=p, t=t: step_case(p, t)) for p in STEP_PLANS for t in SLAB_TARGETS}
CASES["step/siren256_bf16/third_set"] = lambda: step_case("siren256_bf16", "third_set")
CASES.update({
    "shard/siren32": shard_case, "reg/siren32": lambda: reg_case("siren32"), "reg/wire": lambda: reg_case("wire"),
    "loss/B1": lambda: loss_case(1), "loss/B257": lambda: loss_case(257), "loss/B16449": lambda: loss_case(16449),
    "loss_multi/B257": loss_multi_case, "tv/3_2_5_8": lambda: tv_case(3, 2, 5, 8), "tv/2_2_2_2": lambda: tv_case(2, 2, 2, 2),
    "tv/254_254_259_300": lambda: tv_case(254, 254, 259, 300, pointwise_only=True),  # R W > 65536: a lane loops twice
    "center_pairs": center_case, "encode": encode_case, "shuffle/n1": lambda: shuffle_case(1),
    "shuffle/n257": lambda: shuffle_case(257), "shuffle/n65537": lambda: shuffle_case(65537),
    "image_metrics/7x7": lambda: metrics_case(7, 7), "image_metrics/40x37": lambda: metrics_case(40, 37),
    "display/2x9x11": display_case, "band_stats/n1025": bands_case, "coil_gram/3x129": coil_gram_case,
})


def run_case(name):
    res = CASES[name]()
    torch.cuda.synchronize()
    return res


def record(lib_path, commit, out_path, python=sys.executable):
    """The table of the library at ``lib_path`` (built from ``commit``), taken twice in fresh processes; a case whose
    two tables differ is not deterministic: it is reported and left out."""
    import subprocess
    runs = []
    for _ in range(2):
        env = dict(os.environ, INR_LIB_PATH=os.path.abspath(lib_path))
        p = subprocess.run([python, os.path.abspath(__file__)], env=env, capture_output=True, text=True, check=True)
        runs.append(json.loads(p.stdout.splitlines()[-1]))
    cases = {k: v for k, v in runs[0].items() if runs[1].get(k) == v}
    unstable = sorted(set(runs[0]) - set(cases))
    with open(out_path, "w") as f:
        json.dump({"producer_commit": commit, "not_deterministic": unstable, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    return cases, unstable


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "mri-implicit-neural-representations_amd"))
    print(json.dumps({name: run_case(name) for name in CASES}, sort_keys=True))
