"""Deep complex-Gabor networks at full width, held to float64: the case table and the criterion.
tests/test_deep_gabor_host.py (CPU) checks that every case lands on its build, that the oracle is a fair judge there and
that the criterion bites; tests/test_gpu_deep_gabor.py runs the kernels against it.  A plain module, as
tests/matrix_cases.py is, whose Prep / reference / make_mask this table reuses.

Why a table of its own: tests/test_gpu_widths.py::_check(plain=False) accepts FACTOR x the oracle's own fp32-to-float64
distance, and nothing caps that distance -- 3e-3 per tensor for WIRE 256 at omega_0 30 / scale 15, 1.4e-4 at 10 / 5.
Here omega_0 = 1 and scale = 0.5 (first and hidden) put the fp32 oracle within 2.5e-6 of float64, so the project's plain
criterion applies: 1e-5 on output, loss and flat gradient, 2e-5 on every parameter tensor.  The tests at 30 / 15 and
10 / 5 stay as they are: they cover large sine, cosine and exp arguments; these cover what lives BETWEEN the layers of
the two-waves-per-group kernels (WIRE nb12, WIRE2D nb16) -- the per-layer stash slots, the dX chain through several Gabor
Jacobians, the batch dW GEMM with several complex items, its K-chunks over ragged tiles, the padded rows 362..383 of
WIRE's 181 complex features, the complex re-pack after Adam.

A case = (family, depth, last activation, omega_0, scale, loss, mask, NaN in the unsampled rows, B).  Width 256, three
coordinates in, two outputs.  ``network_depth`` counts the hidden complex layers, every one of which is an item of the
batch GEMM (inr_plan.hip::dw_gemm_items, l = 1 .. D - 2 with D = depth + 2 Linear layers): depths 2, 3, 4 give WIRE 2, 3, 4
items and WIRE2D, whose orth Linear is an item too, 4, 6, 8.  ``B`` is symbolic -- tile size, persistent grid and the
GEMM's chunking come from the plan:
  base   2 TL + 37
  chunk  the smallest B whose dW GEMM runs at least 2 tiles per chunk with a ragged last chunk and a ragged last tile
  grid   max_blocks TL + TL + 1: a second round of the persistent grid, ragged; here the step is the split one
         (part of the GEMM beside the partial round)

Everything is a pure function of the case (generators seeded with a hash of its id)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import List, Tuple

import torch

import matrix_cases as MC

WIDTH, IN_F, OUT_F = 256, 3, 2
# the project's plain criterion, against float64 (tests/test_gpu_widths.py::_check plain, tests/test_gpu_layers.py::_hold)
LIMITS = dict(out=1e-5, loss=1e-5, grad=1e-5, tensor=2e-5)
LIMITS_HDR = dict(out=1e-5, loss=2e-5, grad=2e-5)  # tests/test_gpu_matrix.py holds HDR to 2e-5 against the fp32 oracle
# what the fp32 oracle itself must keep to float64 for that criterion to be the device's alone (test_matrix_host's cap)
ORACLE_CAP = dict(out=2.5e-6, grad=2.5e-6, tensor=5e-6, grad_hdr=5e-6)


@dataclass(frozen=True)
class Case:
    family: str          # WIRE (nb12: 181 complex features = 362 of 384 rows) | WIRE2D (nb16: 256 = 512 rows)
    depth: int           # hidden complex layers
    last: str = ""       # "" | ctanh (WIRE2D's last_tanh)
    omega: float = 1.0   # first_omega_0 = hidden_omega_0
    scale: float = 0.5
    loss: str = "L2"     # L2 | HDR
    mask: str = "none"   # none | random (about 0.6)
    nan: bool = False    # the device copy of gt carries NaN in the unsampled rows
    B: str = "base"      # base | chunk | grid

    @property
    def id(self) -> str:
        return "-".join(str(v) for v in (self.family, f"d{self.depth}", self.last or "dflt", f"w{self.omega:g}",
                                         f"s{self.scale:g}", self.loss, self.mask + ("+nan" if self.nan else ""),
                                         f"B{self.B}"))

    @property
    def nb(self) -> int:
        return 12 if self.family == "WIRE" else 16

    @property
    def name(self) -> str:
        """the family as the commit message counts it"""
        return self.family + ("-tanh" if self.last else "")


FAMILIES = [("WIRE", ""), ("WIRE2D", ""), ("WIRE2D", "ctanh")]


def all_cases() -> List[Case]:
    cases: List[Case] = []
    for fam, last in FAMILIES:
        for d in (2, 3, 4):
            cases.append(Case(fam, d, last))
        cases.append(Case(fam, 4, last, B="chunk"))
        # the depth-4 base case under a random mask, with NaN behind the mask, and under the HDR loss
        cases.append(Case(fam, 4, last, mask="random"))
        cases.append(Case(fam, 4, last, mask="random", nan=True))
        cases.append(Case(fam, 4, last, loss="HDR"))
    cases.append(Case("WIRE", 4, omega=2.0, scale=1.0))
    cases.append(Case("WIRE", 3, B="grid"))
    cases.append(Case("WIRE2D", 2, B="grid"))  # (its oracle pair, 16 449 rows, takes about a second on 16 cores)
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = all_cases()


# ---------------------------------------------------------------------------------------------------------------------
# batch sizes from the plan
# ---------------------------------------------------------------------------------------------------------------------
def gemm_chunks(engine, B: int) -> Tuple[int, int, int]:
    """(tiles, chunks, tiles per chunk) of the batch dW GEMM of an unsplit step (B within one round of the grid).
    Chunks = the slabs of engine.workspace(B) behind the launch grid's; dw_gemm_chunk's rule is tiles_per_chunk =
    ceil(tiles / target), chunks = ceil(tiles / tiles_per_chunk), with target = the most tiles that still get a chunk
    each -- read off the plan here, not restated as a number."""
    TL = engine.tile_rows

    def chunks(rows):
        nt, nb = engine.launch_dims(rows)
        assert nt <= nb, "split steps chunk two launches"
        return nt, engine.workspace(rows)[1] - nb

    target = 1
    while chunks((target + 1) * TL) == (target + 1, target + 1):
        target += 1
    nt, n_chunks = chunks(B)
    tpc = -(-nt // target)
    assert n_chunks == -(-nt // tpc), (nt, n_chunks, tpc, target)
    return nt, n_chunks, tpc


def chunk_rows(engine) -> int:
    TL = engine.tile_rows
    for nt in range(2, engine.max_blocks + 1):
        B = (nt - 1) * TL + 1  # the fewest rows with nt tiles: the last tile holds one row
        _, _, tpc = gemm_chunks(engine, B)
        if tpc >= 2 and nt % tpc != 0:
            return B
    raise AssertionError("no batch within one round of the grid chunks its dW GEMM raggedly")


def rows(case: Case, engine) -> int:
    TL = engine.tile_rows
    if case.B == "chunk":
        return chunk_rows(engine)
    return {"base": 2 * TL + 37, "grid": engine.max_blocks * TL + TL + 1}[case.B]


# ---------------------------------------------------------------------------------------------------------------------
# what a case is made of
# ---------------------------------------------------------------------------------------------------------------------
def net_of(case: Case) -> dict:
    return dict(network_input_size=IN_F, network_output_size=OUT_F, network_depth=case.depth, network_width=WIDTH,
                first_omega_0=case.omega, hidden_omega_0=case.omega, scale=case.scale, last_tanh=case.last == "ctanh")


def prepare(case: Case) -> MC.Prep:
    """a matrix_cases.Prep (model on the CPU, plan created without a GPU, inputs, mask, targets): MC.reference and
    tests/test_gpu_matrix.py::Run take it as they take the matrix's own"""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    p = MC.Prep()
    p.case, p.net = case, net_of(case)
    seed = zlib.crc32(case.id.encode())
    torch.manual_seed(seed)
    p.encB = p.bounds = p.dist = p.cons = None
    p.model = {"WIRE": M.WIRE, "WIRE2D": M.WIRE2D}[case.family](p.net)
    if case.loss == "HDR":
        # half the initial output layer (matrix_cases.prepare takes a quarter for these families' non-L2 cases): HDR's
        # gradient divides by |out - gt| >= 0.05, so the oracle's own fp32 output error counts |out| / 0.05 times --
        # at full size it misses the cap on the flat gradient, at a quarter the output rms falls under 0.1
        with torch.no_grad():
            for t in p.model._flat_params[-2:]:
                t.mul_(0.5)
    p.sd = {k: v.clone() for k, v in p.model.state_dict().items()}
    p.engine = p.model._make_engine(L.INPUT_X, 0)
    p.TL = p.engine.tile_rows
    p.B = rows(case, p.engine)
    g = torch.Generator().manual_seed(seed + 1)
    p.x = torch.rand(p.B, IN_F, generator=g) * 2 - 1
    p.mask = MC.make_mask(case.mask, p.B, p.TL, g)
    p.count = p.B if p.mask is None else int(p.mask.sum())
    p.hdr_A = 0.0
    if case.loss == "HDR":
        # A of HDRLoss_FF is a mean over all rows; gt away from the outputs, as matrix_cases.prepare places it (HDR's
        # gradient has a pole at out = gt)
        f = torch.exp(-(p.x[:, 1] ** 2 + p.x[:, 2] ** 2) / (2 * MC.HDR_OPTS["hdr_ff_sigma"] ** 2))
        p.hdr_A = float(torch.mean((1 - f) ** 2))
        out = MC.forward(p, torch.float64)[0].detach().float()
        sign = torch.randint(0, 2, (p.B, OUT_F), generator=g) * 2 - 1
        p.gt = out + (0.05 + 0.25 * torch.rand(p.B, OUT_F, generator=g)) * sign
    else:
        p.gt = torch.randn(p.B, OUT_F, generator=g) * 0.2
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def measure(case: Case, r64, out, loss, grad) -> List[Tuple[str, float, float]]:
    """[(what, error against float64, limit)] of an output [1, B, out_f], a loss and a live flat gradient against
    r64 = MC.reference(p, torch.float64): output, loss and flat gradient, and for the L2 loss every parameter tensor with
    a gradient (a bias vector is a thousandth of the flat norm; the tensor index counts the live ones in layout order)"""
    lim = LIMITS_HDR if case.loss == "HDR" else LIMITS
    l64 = float(r64[1])
    res = [("out", rel_l2(out, r64[0]), lim["out"]), ("loss", abs(float(loss) - l64) / abs(l64), lim["loss"]),
           ("grad", rel_l2(grad, r64[2]), lim["grad"])]
    assert grad.numel() == r64[2].numel()
    off = 0
    for i, g64 in enumerate(r64[3]):
        n = g64.numel()
        if "tensor" in lim and float(g64.norm()) > 0:
            res.append((f"tensor{i}", rel_l2(grad[off:off + n], g64), lim["tensor"]))
        off += n
    return res


def verdict(case: Case, r64, out, loss, grad) -> List[Tuple[str, float, float]]:
    """the measurements that miss their limit (a NaN misses it)"""
    return [m for m in measure(case, r64, out, loss, grad) if not m[1] <= m[2]]


def judge(case: Case, r64, out, loss, grad, tag: str = ""):
    bad = verdict(case, r64, out, loss, grad)
    assert not bad, (case.id + tag, bad)
