"""The conformance matrix's case table: tests/test_matrix_host.py (CPU) checks that every case lands on the build it names
and that the oracle is well-conditioned there; tests/test_gpu_matrix.py runs the kernels against this oracle and imports the same
table (a plain module, not a conftest, so that both see one definition).

A case = (sweep, family, build, width, depth, size, input, out_features, last activation, loss, mask kind, B).  One axis
is swept at a time around a base case per build (out 2, family's default output, L2, no mask, three tiles with a ragged
last one); shapes are the smallest that still select each kernel instantiation: depth 3 (2 in the tile-edge sweep, WIRE 1),
encoder size 8 (32 where the row-split and bf16 kernels need a multiple of 32), the widths below.  ``B`` is symbolic -- the
tile size and the persistent grid come from the plan (engine.tile_rows, engine.max_blocks), never from numbers here.

Everything is a pure function of the case: models, inputs, masks and targets are drawn from generators seeded with a
hash of the case's id, so every module that imports the table sees the same numbers."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace
from typing import List, Optional

import torch

import oracle as O

HDR_OPTS = dict(hdr_eps=1e-3, hdr_ff_sigma=1.0, hdr_ff_factor=0.5)
CONS_W = 0.1           # ConsistencyLoss weight of the multiscale loop (train_kspace_multiscale.py:179)
BOUNDS = (0.2, 0.9)    # (lo, hi) of every BoundedLinear / consistency disc: dist = |(y, x)| of rows in [-1,1]^2 lies on both sides
MFN = ("Fourier", "Gabor", "MultiscaleKFourier", "BoundedFourier")
MULTI = ("MultiscaleKFourier", "BoundedFourier")


@dataclass(frozen=True)
class Case:
    sweep: str           # out | act | mask | nan | edge | loss
    family: str          # SIREN | FFN | WIRE | WIRE2D | Fourier | Gabor | MultiscaleKFourier | BoundedFourier
    build: str           # nb<blocks>[-rs0|-rs1|-512] | bf16-<width>: the kernel instantiation the case must land on
    width: int
    depth: int
    size: int            # encoder size E (input "gauss": in_features = 2E) or in_features (input "x")
    input: str = "gauss"
    out_f: int = 2
    last: str = ""       # "" = the family's default (SIREN linear, FFN sigmoid, WIRE linear); tanh | sin | sigmoid | ctanh
    loss: str = "L2"
    mask: str = "none"   # none | random | tile | one
    B: str = "base"      # base (2 TL + 37) | 1 | TL-1 | TL | TL+1 | grid (max_blocks TL + TL + 1)

    @property
    def id(self) -> str:
        return "-".join(str(v) for v in (self.sweep, self.family, self.input, self.build, f"w{self.width}", f"d{self.depth}",
                                         f"s{self.size}", f"o{self.out_f}", self.last or "dflt", self.loss, self.mask,
                                         f"B{self.B}"))

    @property
    def bf16(self) -> bool:
        return self.build.startswith("bf16")

    @property
    def nb(self) -> int:
        """32-row blocks of the hidden images in the build the case names"""
        return 8 if self.bf16 else int(self.build.split("-")[0][2:])

    @property
    def tile_rows(self) -> int:
        """the 12- and 16-block kernels run two waves per coordinate group on 64-coordinate tiles"""
        return 64 if self.nb in (12, 16) else 128

    @property
    def rs(self) -> Optional[str]:
        """INR_RS the case runs under (the nb8 plans behind the fused gauss encoder own two fused kernels)"""
        return {"nb8-rs0": "0", "nb8-rs1": "1"}.get(self.build)

    @property
    def gemm(self) -> bool:
        """weight gradients of the fused step from the batch GEMM (inr_sizes.step_save_by_tile): the bf16 plans; the wide
        filter kernel; 8 / 12 / 16-block MLP and WIRE plans with a layer the GEMM covers (the first one behind the fused
        encoder, every hidden-to-hidden one); WIRE2D only in its 16-block build"""
        if self.bf16:
            return True
        if self.family in MFN:
            return self.nb == 16
        if self.family == "WIRE2D":
            return self.nb == 16
        if self.family == "WIRE":
            return self.nb in (8, 12)  # depth 1 = one hidden complex layer
        return self.nb in (8, 16) and (self.input == "gauss" or self.depth >= 3)

    @property
    def plain(self) -> bool:
        """SIREN with a linear / tanh output and FFN: the project's plain 1e-5 criterion.  Everything else (complex Gabor
        layers, filter networks, sin(30 z) on the output) is held to FACTOR x the oracle's own fp32 error."""
        return self.family in ("SIREN", "FFN") and self.last != "sin" and not self.bf16


# (build, width, size)
MLP_GAUSS = [("nb1", 17, 8), ("nb2", 33, 8), ("nb4", 100, 8), ("nb8-rs0", 130, 32), ("nb8-rs1", 130, 32), ("nb16", 300, 8),
             ("nb16-512", 512, 8)]
MLP_X = [("nb1", 17, 3), ("nb8", 130, 60), ("nb16", 300, 60)]   # in_features 3 and 60: no multiple of 8
WIRE = [("nb2", 24), ("nb4", 64), ("nb8", 100), ("nb12", 200)]  # int(width / sqrt 2) = 16, 45, 70, 141 complex features
WIRE2D = [("nb2", 8), ("nb4", 40), ("nb8", 72), ("nb16", 136)]  # complex features = width
MFN_BUILDS = [("nb1", 20), ("nb16", 260)]                       # inr_mfn_impl.h | inr_mfn_wide_impl.h
BF16 = [("bf16-160", 160, 32), ("bf16-256", 256, 32)]


def _bases() -> List[Case]:
    """one base case per build: (sweep filled in by the caller)"""
    out = []
    for b, w, e in MLP_GAUSS:
        out.append(Case("", "SIREN", b, w, 3, e))
    for b, w, k in MLP_X:
        out.append(Case("", "SIREN", b, w, 3, k, input="x"))
    for b, w, e in MLP_GAUSS:  # the sigmoid epilogue on every build SIREN's runs on
        out.append(Case("", "FFN", b, w, 3, e))
    for b, w, k in MLP_X:
        out.append(Case("", "FFN", b, w, 3, k, input="x"))
    for b, w in WIRE:
        out.append(Case("", "WIRE", b, w, 1, 3, input="x"))
    for b, w in WIRE2D:
        out.append(Case("", "WIRE2D", b, w, 1, 3, input="x"))
    for fam in MFN:
        for b, w in MFN_BUILDS:
            out.append(Case("", fam, b, w, 3, 8))
    for b, w, e in BF16:
        out.append(Case("", "SIREN", b, w, 3, e))
    return out


def all_cases() -> List[Case]:
    cases: List[Case] = []
    bases = _bases()
    # 1. output sizes (out 2 = the base case of every other sweep); WIRE2D also with the complex tanh, which keeps both
    #    rows of a complex pair: one and two outputs
    for c in bases:
        for o in (1, 2, 3, 4):
            cases.append(replace(c, sweep="out", out_f=o))
        if c.family == "WIRE2D":
            for o in (1, 2):
                cases.append(replace(c, sweep="out", out_f=o, last="ctanh"))
    # 2. last activation: SIREN tanh and network_last_linear False (linear is the base, FFN's sigmoid its own base);
    #    bf16 also a sigmoid, which only a hand-made descriptor reaches
    for c in bases:
        if c.family == "SIREN" and c.input == "gauss" and c.build in ("nb1", "nb8-rs0", "nb8-rs1", "nb16"):
            cases += [replace(c, sweep="act", last=a) for a in ("tanh", "sin")]
        if c.bf16:
            cases += [replace(c, sweep="act", last=a) for a in ("tanh", "sin", "sigmoid")]
    # 3. masks, every build; one case per family with NaN in the unsampled rows of gt
    for c in bases:
        cases += [replace(c, sweep="mask", mask=m) for m in ("random", "tile", "one")]
    seen = set()
    for c in bases:
        key = "bf16" if c.bf16 else c.family
        if key not in seen and c.build not in ("nb1", "nb2"):
            seen.add(key)
            cases.append(replace(c, sweep="nan", mask="random"))
    # 4. tile edges, every build, depth 2 -- the bf16 kernels start at 3 layers.  FFN stays out of this sweep alone: its kernels
    #    are SIREN's templates instantiated with another hidden activation (HACT), the tile loop, the ragged tail and the
    #    persistent grid are the same source lines, and the five batch sizes of ten more builds cost the most oracle time
    for c in bases:
        if c.family != "FFN":
            d = c.depth if (c.family in ("WIRE", "WIRE2D") or c.bf16) else 2
            cases += [replace(c, sweep="edge", depth=d, B=b) for b in ("1", "TL-1", "TL", "TL+1", "grid")]
    # 5. losses: pointwise on nb1, nb16 and one WIRE2D build; multi-head with the consistency term on the wide filter kernel
    for c in bases:
        if (c.family, c.input, c.build) in (("SIREN", "gauss", "nb1"), ("SIREN", "gauss", "nb16"), ("WIRE2D", "x", "nb4"),
                                            ("MultiscaleKFourier", "gauss", "nb16")):
            cases += [replace(c, sweep="loss", loss=k) for k in ("L1", "tanh", "LogSpace", "HDR", "MSLE")]
            cases.append(replace(c, sweep="loss", loss="HDR", mask="random"))
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = all_cases()


def by_sweep(*sweeps: str) -> List[Case]:
    return [c for c in CASES if c.sweep in sweeps]


# ---------------------------------------------------------------------------------------------------------------------
# what a case is made of
# ---------------------------------------------------------------------------------------------------------------------
def rows(case: Case, TL: int, max_blocks: int) -> int:
    return {"base": 2 * TL + 37, "1": 1, "TL-1": TL - 1, "TL": TL, "TL+1": TL + 1, "grid": max_blocks * TL + TL + 1}[case.B]


def make_mask(kind: str, B: int, TL: int, g: torch.Generator) -> Optional[torch.Tensor]:
    """none | random (about 0.6) | tile (zeros over the whole second tile, ones over the ragged last one) | one (a single
    sampled row, in the ragged last tile)"""
    if kind == "none":
        return None
    m = torch.rand(B, generator=g) < 0.6
    if kind == "tile":
        assert B > 2 * TL
        m[TL:2 * TL] = False
        m[2 * TL:] = True
    elif kind == "one":
        m[:] = False
        m[max(0, B - 2)] = True
    if not bool(m.any()):
        m[0] = True
    return m


def net_of(case: Case) -> dict:
    in_f = 2 * case.size if case.input == "gauss" else case.size
    net = dict(network_input_size=in_f, network_output_size=case.out_f, network_depth=case.depth, network_width=case.width)
    if case.family == "SIREN":
        net.update(last_tanh=case.last == "tanh", network_last_linear=case.last != "sin")
    if case.family in ("WIRE", "WIRE2D"):
        net.update(first_omega_0=10, hidden_omega_0=10, scale=5, last_tanh=case.last == "ctanh")
    return net


class Prep:
    """model (CPU), plan, inputs and targets of one case"""


def prepare(case: Case) -> Prep:
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    from inr_mi355x import mfn
    from inr_mi355x.engine import MFNEngine, MLPEngine
    p = Prep()
    p.case, p.net = case, net_of(case)
    seed = zlib.crc32(case.id.encode())
    torch.manual_seed(seed)
    p.encB = None
    if case.input == "gauss":  # scale 1: phases of a few revolutions, so the fp32 oracle's own features stay at 1e-7
        p.enc = M.Positional_Encoder(dict(embedding="gauss", scale=1, embedding_size=case.size, coordinates_size=3), "cpu")
        p.encB = p.enc.B.clone()
    p.bounds = [BOUNDS] * case.depth if case.family == "BoundedFourier" else None
    cls = {"SIREN": M.SIREN, "FFN": M.FFN, "WIRE": M.WIRE, "WIRE2D": M.WIRE2D, "Fourier": mfn.FourierNet,
           "Gabor": mfn.GaborNet, "MultiscaleKFourier": mfn.MultiscaleKFourier}.get(case.family)
    p.model = mfn.MultiscaleBoundedFourier(p.net, boundaries=p.bounds) if cls is None else cls(p.net)
    if case.loss != "L2" and case.family in ("WIRE", "WIRE2D"):
        # outputs of O(1) leave 1 + out of MSLE without a sign: a quarter of the initial output layer keeps them inside (-1, 1)
        with torch.no_grad():
            for t in p.model._flat_params[-2:]:
                t.mul_(0.25)
    p.sd = {k: v.clone() for k, v in p.model.state_dict().items()}
    # the plan: created without a GPU; a GPU test binds it to the model's flat parameters
    if case.family in MFN:
        kind = {"Fourier": L.KIND_FOURIER, "Gabor": L.KIND_GABOR, "MultiscaleKFourier": L.KIND_MSFOURIER,
                "BoundedFourier": L.KIND_MSBOUNDED}[case.family]
        p.engine = MFNEngine(kind, p.net["network_input_size"], case.width, case.depth, case.out_f, case.size, p.bounds)
    elif case.family in ("WIRE", "WIRE2D"):
        p.engine = p.model._make_engine(L.INPUT_X, 0)
    elif case.last == "sigmoid" and case.family == "SIREN":  # no model class maps to it: a descriptor made by hand
        d = p.model._dims
        p.engine = MLPEngine(L.KIND_SIREN, d[0], d[1], len(d) - 1, d[-1], L.ACT_SIGMOID, L.INPUT_GAUSS, case.size, 30.0,
                             precision=L.PRECISION_BF16 if case.bf16 else L.PRECISION_F32)
    else:
        mode, E = (L.INPUT_GAUSS, case.size) if case.input == "gauss" else (L.INPUT_X, 0)
        p.engine = p.model._make_engine(mode, E, L.PRECISION_BF16 if case.bf16 else L.PRECISION_F32)
    p.TL = p.engine.tile_rows
    p.B = rows(case, p.TL, p.engine.max_blocks)
    g = torch.Generator().manual_seed(seed + 1)
    p.x = torch.rand(p.B, 3 if case.input == "gauss" or case.family in ("WIRE", "WIRE2D") else case.size, generator=g) * 2 - 1
    p.dist = torch.sqrt(p.x[:, 1] ** 2 + p.x[:, 2] ** 2) if case.family in MFN else None
    p.mask = make_mask(case.mask, p.B, p.TL, g)
    p.count = p.B if p.mask is None else int(p.mask.sum())
    p.hdr_A = 0.0
    if case.loss == "HDR":  # A of HDRLoss_FF: a mean over ALL rows of the batch (the reference passes the unmasked coordinates)
        f = torch.exp(-(p.x[:, 1] ** 2 + p.x[:, 2] ** 2) / (2 * HDR_OPTS["hdr_ff_sigma"] ** 2))
        p.hdr_A = float(torch.mean((1 - f) ** 2))
    p.cons = None
    if case.loss != "L2" and case.family in MULTI:  # the multi-head form: consistency between consecutive heads
        n_heads = len([s for s in (1, 3, 5, 7) if s <= case.depth])
        p.cons = [(0.0, BOUNDS[0] + 0.3 * i) for i in range(n_heads)]
    if case.loss == "L2":
        p.gt = (torch.rand(p.B, case.out_f, generator=g) * 0.5 if case.family == "FFN"
                else torch.randn(p.B, case.out_f, generator=g) * 0.2)
    else:
        # away from the outputs: HDR's gradient 2 log(|e| / den) e / |e|^2 has a pole at e = 0 (tests/test_gpu_rs.py), L1's a jump
        # (MSLE takes log(1 + .) of both: its targets lie above the outputs)
        # and a multi-head case's above every head's)
        out = torch.stack(forward(p, torch.float64)).detach().float()
        sign = torch.randint(0, 2, (p.B, case.out_f), generator=g) * 2 - 1
        above = case.loss == "MSLE" or out.shape[0] > 1
        p.gt = out.max(0)[0] + (0.05 + 0.25 * torch.rand(p.B, case.out_f, generator=g)) * (1 if above else sign)
    return p


def plan_cons(p: Prep):
    """ConsistencySpec of a multi-head loss case: pair i compares heads i, i + 1 on the rows outside disc i"""
    from inr_mi355x.engine import ConsistencySpec
    if p.cons is None:
        return None
    inv = []
    for lo, hi in p.cons[:-1]:
        n = int(((p.dist < lo) | (p.dist > hi)).sum())
        inv.append(1.0 / (2.0 * n) if n else 0.0)
    return ConsistencySpec(CONS_W, p.cons, inv + [0.0], 2)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle: forward, loss and per-tensor gradients in one dtype
# ---------------------------------------------------------------------------------------------------------------------
def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _params(p: Prep, dtype):
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    frozen = ("omega_0", "scale_0")
    keys_all = [k for k in p.sd if not k.endswith(frozen)]  # state_dict order = the flat layout's order
    live = getattr(p.model, "_live", [True] * len(keys_all))
    assert len(live) == len(keys_all) == len(p.model._layout)
    keys = [k for k, lv in zip(keys_all, live) if lv]
    params = {}
    for k, v in p.sd.items():
        v = v.to(cd) if v.is_complex() else v.to(dtype)
        params[k] = v.clone().requires_grad_(True) if k in keys else v
    return params, keys


def forward(p: Prep, dtype, params=None) -> List[torch.Tensor]:
    """heads of the oracle's forward, [B, out_f] each"""
    kind = p.case.family
    if params is None:
        params, _ = _params(p, dtype)
    x = p.x.to(dtype) if p.encB is None else O.encode(p.x.to(dtype), p.encB.to(dtype), "gauss")
    outs = O.model_forward(kind, params, x, p.net, dist_to_center=None if p.dist is None else p.dist.to(dtype),
                           boundaries=p.bounds)
    return [o.contiguous() for o in (outs if isinstance(outs, list) else [outs])]


def pointwise(name: str, o: torch.Tensor, g: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    if name == "L2":
        return O.loss_l2_half(o, g)
    if name == "L1":
        return O.loss_l1_half(o, g)
    if name == "tanh":
        return O.loss_tanh(o, g)[0]
    if name == "LogSpace":
        return O.loss_logspace(o, g, HDR_OPTS)
    if name == "HDR":
        return O.loss_hdr(o, g, coords, HDR_OPTS)[0]
    if name == "MSLE":
        return 0.5 * O.loss_msle(o, g)
    raise NotImplementedError(name)


def reference(p: Prep, dtype):
    """(out [heads, B, out_f], loss, flat gradient of the live tensors in layout order, [per-tensor gradients]) -- the
    first three as tests/test_gpu_widths.py::_ref returns them; the oracle indexes out[mask], gt[mask] as the reference
    does (train.py:172-177), the consistency term sees every row"""
    params, keys = _params(p, dtype)
    outs = forward(p, dtype, params)
    gt, coords = p.gt.to(dtype), p.x.to(dtype)
    loss = 0
    for o in outs:
        o_, g_ = (o, gt) if p.mask is None else (o[p.mask], gt[p.mask])
        loss = loss + pointwise(p.case.loss, o_.contiguous(), g_.contiguous(), coords)
    if p.cons is not None:
        loss = loss + CONS_W * O.loss_consistency(outs, p.dist.to(dtype), p.cons)
    grads = [_real(g).reshape(-1) for g in torch.autograd.grad(loss, [params[k] for k in keys])]
    return torch.stack([o.detach() for o in outs]), loss.detach(), torch.cat(grads), grads
