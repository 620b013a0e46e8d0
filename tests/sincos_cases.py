"""The sine / cosine isolation cases: tests/test_sincos_host.py (CPU) checks that every case lands on the build it names and
that its network really is one transcendental of a known fp32 argument; tests/test_gpu_sincos.py runs the shipped kernels
and compares every output element with float64 sin / cos of that argument (a plain module, not a conftest, as
tests/matrix_cases.py is).

A case = (call site, build, argument range).  Its network is made by hand so that the public forward returns
out[r, o] = sin or cos of ONE fp32 argument t[r, o] and nothing else: one-hot weights of +-1, zero biases, so every
product and sum between the transcendental and the output is exact.  ``depth`` below counts Linear layers for SIREN / FFN
(2 = one hidden activation) and hidden complex layers for WIRE / WIRE2D (0 = the first Gabor layer and the final Linear),
as the plan does: each network has exactly one activation layer.

site    network                                                  argument (restated in numpy float32)
feat    FFN-kind descriptor, ReLU hidden, identity output,       ph = fl(fl(2 pi) x_a) 2^k: encB rows hold one power of
        fused gauss encoder; hidden units +f, -f of a feature,   two 2^0..2^7 on one axis, so the phase is exact in any
        out = relu(f) - relu(-f) = f; four features per call     evaluation order; |ph| reaches 2^7 * 2 pi = 804 rad
sin     SIREN on x, linear output, first-layer rows one-hot 1    t = fl(30 z), z = x[r, col]: the one fp32 rounding of
                                                                 act_fwd<ACT_SIN> (networks.py:96)
wire    WIRE, scale_0 = 0, real first layer (zero imaginary      t = fl(10 a), a = x[r, col] (act_gabor / wire_epilogue)
wire2d  rows), zero scale_orth: the envelope is exp(-0) = 1;     the same through act_gabor2d / wire2d_epilogue
        output weight 1 -> cos, -j -> sin
fourier FourierNet / GaborNet on x, depth 1: filter 0 is zero,   t = x[r, col] itself: weight 1, zero bias, nothing is
gabor   linear.0 = (0, bias 1), so the stage-1 product is        rounded before the sine (mfn_epilogue, both kernels)
        sin(u) * 1; mu = gamma = 0: envelope exp(-0) = 1

Not in the table, and why:
* the row-split fused step (inr_mlp_rs_impl.h: rs_gen's layer-0 phases, rs_act_park's hidden sine).  Only the fused step
  launches that kernel; it returns a loss and a gradient, no output rows, and forward calls of an nb8 gauss plan run
  inr_mlp_kernel under either INR_RS (inr_api.hip: inr_forward).  The nb8 gauss plan is therefore in the table once, as
  "nb8-rs0".  (rs_act_park reduces fl(w0 z) in radians with sincos_cw's constants, not a revolutions accumulator.)
* act_ctanh.  Re tanh(a + jb) = sinh 2a / (cosh 2a + cos 2b): at a = 0 it is 0 for every b, and at a != 0 the output
  carries expf's and the division's roundings as well -- no choice of weights leaves the cosine alone.
* the stage-0 filter of the filter networks (mfn_epilogue<FIRST>): reading it through stage 1 needs a second filter that
  is exactly 1, which sin(fl(pi / 2)) is not.  Stage 1 runs the same sincos_cw line.
* the multiscale kinds: the single-head form already isolates the filter.

Rows: 2 * tile_rows + 37 (a ragged last tile, as the matrix's base case), the last ones fixed: the zero phase, the largest
of the range, and the fp32 arguments next to k 2 pi and (k + 1/2) 2 pi (the nearest z and both its neighbours), all with
both signs.  Random rows come from a generator seeded with the case id."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

import matrix_cases as MC

W0_SIREN = 30.0
OMEGA_WIRE = 10.0
LO_MAX, HI_MAX = 300.0, 8192.0
TWO_PI32 = np.float32(6.283185307179586)
# the bounds of tests/test_gpu_sincos.py (none fitted): sincos_cw's documented error (inr_device.h) | the one-transcendental
# feature form: + one more fp32 rounding of an argument below one revolution, 2 pi * 2^-25
BOUND_CW = 3.8e-7
BOUND_FEAT = 3.8e-7 + 2.0 * np.pi * 2.0 ** -25


@dataclass(frozen=True)
class Case:
    site: str        # feat | sin | wire | wire2d | fourier | gabor
    build: str       # the kernel instantiation the case must land on (tests/matrix_cases.py's names)
    width: int
    size: int        # encoder size E (feat) or in_features
    rng: str         # enc (feat: |ph| <= 2^7 fl(2 pi)) | lo (|t| <= 300) | hi (300 < |t| <= 8192)

    @property
    def id(self) -> str:
        return "-".join((self.site, self.build, f"w{self.width}", f"s{self.size}", self.rng))

    @property
    def nb(self) -> int:
        return int(self.build.split("-")[0][2:])

    @property
    def tile_rows(self) -> int:
        return 64 if self.nb in (12, 16) else 128

    @property
    def bound(self) -> float:
        return BOUND_FEAT if self.site == "feat" else BOUND_CW

    @property
    def interval(self):
        """(lo, hi]: where the largest |argument| of the case lies; every row of a "hi" case lies in it"""
        return {"enc": (LO_MAX, 128 * float(TWO_PI32)), "lo": (0.99 * LO_MAX, LO_MAX), "hi": (LO_MAX, HI_MAX)}[self.rng]


# x-input widths per build (matrix_cases.MLP_X names nb1, nb8, nb16; the other three builds run the same template)
SIN_X = [("nb1", 17, 3), ("nb2", 33, 3), ("nb4", 100, 60), ("nb8", 130, 60), ("nb16", 300, 60), ("nb16-512", 512, 60)]
MFN_X = [("nb1", 20), ("nb4", 100), ("nb8", 200), ("nb16", 260)]


def all_cases() -> List[Case]:
    cases = [Case("feat", b, w, e, "enc") for b, w, e in MC.MLP_GAUSS if b != "nb8-rs1"]
    for r in ("lo", "hi"):
        cases += [Case("sin", b, w, k, r) for b, w, k in SIN_X]
        cases += [Case("wire", b, w, 3, r) for b, w in MC.WIRE]
        cases += [Case("wire2d", b, w, 3, r) for b, w in MC.WIRE2D]
        for fam in ("fourier", "gabor"):
            cases += [Case(fam, b, w, 4, r) for b, w in MFN_X]
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = all_cases()


# ---------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------
def _f32(v):
    return np.asarray(v, dtype=np.float32)


def restate(case: Case, z: np.ndarray) -> np.ndarray:
    """the fp32 argument of the transcendental for pre-activation z, as the kernel forms it: one fp32 product"""
    w = {"sin": W0_SIREN, "wire": OMEGA_WIRE, "wire2d": OMEGA_WIRE}.get(case.site)
    z = _f32(z)
    return z if w is None else (np.float32(w) * z).astype(np.float32)


def _z_for(case: Case, t: float) -> np.ndarray:
    """the fp32 z whose argument is nearest to t, and both its neighbours"""
    w = {"sin": W0_SIREN, "wire": OMEGA_WIRE, "wire2d": OMEGA_WIRE}.get(case.site, 1.0)
    z = np.float32(t / w)
    return _f32([np.nextafter(z, np.float32(-np.inf)), z, np.nextafter(z, np.float32(np.inf))])


def _fixed_z(case: Case) -> np.ndarray:
    lo, hi = case.interval
    ks = (1, 7, 47) if case.rng == "lo" else (48, 500, 1303)  # 47.5 * 2 pi = 298.5, 1303.5 * 2 pi = 8190.1
    z = [_z_for(case, (k + h) * 2 * np.pi) for k in ks for h in (0.0, 0.5)]
    zmax = _z_for(case, hi)[1]
    while float(restate(case, zmax)) > hi:  # the largest argument of the range that the product reaches
        zmax = np.nextafter(zmax, np.float32(0))
    z = np.concatenate(z + [_f32([zmax])])
    z = np.concatenate([z, -z] + ([_f32([0.0])] if case.rng == "lo" else []))
    t = np.abs(restate(case, z).astype(np.float64))
    assert (t <= hi).all() and (case.rng == "lo" or (t > lo).all())
    return z


def _random_z(case: Case, n: int, cols: int, g: torch.Generator) -> np.ndarray:
    lo, hi = case.interval
    lo = 0.0 if case.rng == "lo" else lo
    u = torch.rand(n, cols, generator=g, dtype=torch.float64).numpy()
    sign = torch.randint(0, 2, (n, cols), generator=g).numpy() * 2.0 - 1.0
    w = {"sin": W0_SIREN, "wire": OMEGA_WIRE, "wire2d": OMEGA_WIRE}.get(case.site, 1.0)
    # 0.1 % inside the interval: the product's rounding cannot step over either end
    t = sign * (lo * 1.001 + u * (hi * 0.999 - lo * 1.001))
    return _f32(t / w)


FEAT_FIXED = (0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(0))), 0.5, float(np.nextafter(np.float32(0.5), np.float32(0))),
              float(np.nextafter(np.float32(0.5), np.float32(1))), 0.25, 0.75, 0.125)


def feat_encB(E: int) -> torch.Tensor:
    """row s: 2^(s % 8) on axis (s + s // 8) % 3, zero elsewhere"""
    B = torch.zeros(E, 3)
    for s in range(E):
        B[s, (s + s // 8) % 3] = 2.0 ** (s % 8)
    return B


def feat_phase(x: np.ndarray, encB: np.ndarray) -> np.ndarray:
    """[rows, E] fp32 phases as fwd_layer0_gauss forms them: xs = fl(fl(2 pi) x); the FMA chain over three axes adds two
    exact zeros to xs_a 2^k, itself exact"""
    xs = (TWO_PI32 * _f32(x)).astype(np.float32)
    ph = np.zeros((x.shape[0], encB.shape[0]), dtype=np.float32)
    for s in range(encB.shape[0]):
        a = int(np.nonzero(encB[s])[0][0])
        ph[:, s] = xs[:, a] * np.float32(encB[s, a])
    return ph


# ---------------------------------------------------------------------------------------------------------------------
# what a case is made of
# ---------------------------------------------------------------------------------------------------------------------
class Prep:
    """engine (plan, created without a GPU), inputs, and per call: the flat parameters, the oracle's state dict, the fp32
    arguments arg[c] [rows, 4] and which function of them each output column is (cos[c] [4] bool)"""


def _units(width: int) -> List[int]:
    """four hidden units spread over the row blocks"""
    return [0, width // 3, (2 * width) // 3, width - 1]


def _cols(in_f: int) -> List[int]:
    return [(i * (in_f - 1)) // 3 for i in range(4)]


def _zero(model):
    with torch.no_grad():
        model._flat.zero_()


def _snapshot(p: Prep, model):
    p.flats.append(model._flat.detach().clone())
    p.sds.append({k: v.detach().clone() for k, v in model.state_dict().items()})


def prepare(case: Case) -> Prep:
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    from inr_mi355x import mfn
    from inr_mi355x.engine import MFNEngine, MLPEngine
    p = Prep()
    p.case = case
    seed = zlib.crc32(case.id.encode())
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    p.flats, p.sds, p.arg, p.cos = [], [], [], []
    p.encB = p.dist = None
    W = case.width
    if case.site == "feat":
        E = case.size
        p.net = dict(network_input_size=2 * E, network_output_size=4, network_depth=2, network_width=W)
        p.family = "FFN-id"  # no model class maps to ReLU hidden + identity output: a descriptor made by hand
        model = M.FFN(p.net)
        p.engine = MLPEngine(L.KIND_FFN, 2 * E, W, 2, 4, L.ACT_ID, L.INPUT_GAUSS, E, W0_SIREN)
        p.encB = feat_encB(E)
        p.B = 2 * p.engine.tile_rows + 37
        fixed = _f32([[s * v] * 3 for v in FEAT_FIXED for s in ((1.0, -1.0) if v else (1.0,))])
        rnd = (torch.rand(p.B - len(fixed), 3, generator=g) * 2 - 1).numpy()
        p.x = torch.from_numpy(np.concatenate([rnd, fixed]))
        ph = feat_phase(p.x.numpy(), p.encB.numpy())
        w0, _, w1, _ = model._flat_params
        for c in range(2 * E // 4):  # call c reads features 4c .. 4c + 3 of [sin | cos]
            _zero(model)
            u0 = (8 * c) % (W - 7)
            with torch.no_grad():
                for i in range(4):
                    f = 4 * c + i
                    w0[u0 + 2 * i, f], w0[u0 + 2 * i + 1, f] = 1.0, -1.0
                    w1[i, u0 + 2 * i], w1[i, u0 + 2 * i + 1] = 1.0, -1.0
            _snapshot(p, model)
            fs = np.arange(4 * c, 4 * c + 4)
            p.arg.append(ph[:, fs % E])
            p.cos.append(fs >= E)
    else:
        in_f = case.size
        units, cols = _units(W), _cols(in_f)
        if case.site in ("wire", "wire2d"):
            hid = W if case.site == "wire2d" else int(W / np.sqrt(2))
            units = [1, 1, hid - 1, hid - 1]  # (cos, sin) of two complex features
            cols = [0, 0, in_f - 1, in_f - 1]
        if case.site == "sin":
            p.family = "SIREN"
            p.net = dict(network_input_size=in_f, network_output_size=4, network_depth=2, network_width=W)
            model = M.SIREN(p.net)
            p.engine = model._make_engine(L.INPUT_X, 0)
        elif case.site in ("wire", "wire2d"):
            p.family = "WIRE" if case.site == "wire" else "WIRE2D"
            p.net = dict(network_input_size=in_f, network_output_size=4, network_depth=0, network_width=W,
                         first_omega_0=OMEGA_WIRE, hidden_omega_0=OMEGA_WIRE, scale=0.0)
            model = (M.WIRE if case.site == "wire" else M.WIRE2D)(p.net)
            p.engine = model._make_engine(L.INPUT_X, 0)
        else:
            p.family = "Fourier" if case.site == "fourier" else "Gabor"
            p.net = dict(network_input_size=in_f, network_output_size=4, network_depth=1, network_width=W)
            model = (mfn.FourierNet if case.site == "fourier" else mfn.GaborNet)(p.net)
            kind = L.KIND_FOURIER if case.site == "fourier" else L.KIND_GABOR
            p.engine = MFNEngine(kind, in_f, W, 1, 4, 0, None, input_mode=L.INPUT_X)
        p.B = 2 * p.engine.tile_rows + 37
        fixed = _fixed_z(case)
        z = np.concatenate([_random_z(case, p.B - len(fixed), in_f, g), np.repeat(fixed[:, None], in_f, axis=1)])
        p.x = torch.from_numpy(z)
        if p.family in ("Fourier", "Gabor"):
            p.dist = torch.zeros(p.B)
        _zero(model)
        sd = dict(model.named_parameters())
        with torch.no_grad():
            for i, (u, k) in enumerate(zip(units, cols)):
                if p.family == "SIREN":
                    sd["model.0.linear.weight"][u, k] = 1.0
                    sd["model.1.linear.weight"][i, u] = 1.0
                elif p.family in ("WIRE", "WIRE2D"):
                    sd["net.0.linear.weight"][u, k] = 1.0
                    sd["net.1.weight"][i, u] = complex(0.0, -1.0) if i % 2 else complex(1.0, 0.0)
                else:
                    sd["linear.0.bias"][:] = 1.0
                    sd["filters.1.linear.weight"][u, k] = 1.0
                    sd["output_linear.weight"][i, u] = 1.0
        _snapshot(p, model)
        p.arg.append(restate(case, z[:, cols]))
        p.cos.append(np.array([case.site in ("wire", "wire2d") and i % 2 == 0 for i in range(4)]))
    p.TL = p.engine.tile_rows
    return p


def expected(p: Prep, c: int) -> np.ndarray:
    """float64 sin / cos of call c's fp32 arguments, [rows, 4]"""
    t = p.arg[c].astype(np.float64)
    return np.where(p.cos[c][None, :], np.cos(t), np.sin(t))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 oracle of the isolation network, and the argument it takes the sine of
# ---------------------------------------------------------------------------------------------------------------------
def oracle_forward(p: Prep, c: int) -> np.ndarray:
    import oracle as O
    sd = {k: (v.to(torch.complex128) if v.is_complex() else v.double()) for k, v in p.sds[c].items()}
    x = p.x.double()
    if p.family == "FFN-id":  # (oracle.model_forward's FFN ends in a sigmoid: the two Linears and the ReLU spelled out)
        f = O.encode(x, p.encB.double(), "gauss")
        h = torch.relu(f @ sd["model.0.weight"].t() + sd["model.0.bias"])
        return (h @ sd["model.2.weight"].t() + sd["model.2.bias"]).numpy()
    return O.model_forward(p.family, sd, x, p.net).numpy()


def oracle_argument(p: Prep, c: int) -> np.ndarray:
    """what the float64 oracle takes the sine of, [rows, 4]: the same products without the fp32 roundings"""
    x = p.x.double().numpy()
    if p.case.site == "feat":
        ph = ((2.0 * np.pi * p.x.double()) @ p.encB.double().t()).numpy()  # oracle.encode's phase
        fs = np.arange(4 * c, 4 * c + 4)
        return ph[:, fs % p.case.size]
    w = {"sin": W0_SIREN, "wire": OMEGA_WIRE, "wire2d": OMEGA_WIRE}.get(p.case.site, 1.0)
    cols = _cols(p.case.size)
    if p.case.site in ("wire", "wire2d"):
        cols = [0, 0, p.case.size - 1, p.case.size - 1]
    return w * x[:, cols]
