"""The batch-level weight-gradient GEMM on the device, element by element against float64 -- ``-m gpu``
(csrc/inr_dw_gemm.hip, csrc/inr_dw_gemm_split.hip, chunked by csrc/inr_layout.hip; cases and reference:
tests/dw_gemm_cases.py, shown sound on the CPU by tests/test_dw_gemm_host.py).

Per case, per layer the GEMM covers, per stored element of dW and db:
    err(g) = |g - g64| / S,  S = |dZ|^T |h|  (sum_c |dZ| for db);   S == 0  =>  g == 0.0 exactly;
    max err(device) <= FACTOR x e_ref,  e_ref = max err of the float32 restatement, FACTOR = 4 (tests/test_gpu_widths.py);
    three-term kernel: max err(split) <= 2 x max err(fp32 kernel), same process, same plan, INR_DW_SPLIT flipped per call
    (tests/test_gpu_dw_split.py's allowance for the six-of-nine products, element by element);
    INR_DW_PLACE=0 gives the three-term kernel's bits; two calls on the same inputs are bitwise equal;
    a one-hot d(loss)/d(out) gives, to the bit, what its coordinate gives alone in a batch of one row.
(e_ref of the one-term sums and the allowance of db: see "the yardstick" in tests/dw_gemm_cases.py.)
No absolute floor.  Routes: 1 forward(save=True) + backward with a chosen d(loss)/d(out); 2 the fused step (its own
chunking: a batch past the persistent grid runs two GEMM launches, the second at tile0 > 0); 3 the split row-split step.
Every case asserts the kernel build and the route it landed on from what the plan reports; the chunk geometry is the restated rule
that the host test holds to inr_plan_workspace.  The measured (e_ref, e_device) pairs go through conftest.record_parity
(profiles/dw_gemm_parity.jsonl is a committed copy of one run).

db of routes 2 and 3 is allowed FACTOR x e_ref + 2 x 3.8e-7 (dw_gemm_cases.db_allowance): the loss makes d(loss)/d(out)
coherent with the Jacobian, and the kernels' sine and cosine (3.8e-7, tests/test_gpu_sincos.py) then stay in the sum; the
measurements that place this outside the GEMM are written next to the yardstick in tests/dw_gemm_cases.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dw_gemm_cases as D  # noqa: E402
import matrix_cases as MC  # noqa: E402
from test_gpu_dw_split import _fp32_kernel  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bound(p, dev):
    """the shape's plan bound (once) to a device copy of its parameters"""
    if getattr(p, "dev_bound", None) is None:
        p.engine.bind(p.model._flat.detach().clone().to(dev))
        p.encB_dev = None if p.encB is None else p.encB.to(dev).contiguous()
        p.dev_bound = True
    return p.engine


class _Device:
    """operands of a case on the device, and the case's route through an engine"""

    def __init__(self, p, o, case, dev):
        self.p, self.o, self.case = p, o, case
        self.mfn = p.shape.family in MC.MFN
        self.x = o.x.to(dev).contiguous()
        self.dist = None if o.dist is None else o.dist.to(dev).contiguous()
        self.dout = None if o.dout is None else o.dout.to(dev).contiguous()
        self.gt = None if o.gt is None else o.gt.to(dev).contiguous()
        self.mask = None if o.mask is None else o.mask.to(torch.uint8).to(dev)

    def run(self, eng, encB, **env):
        """flat gradient (host) of one call under the route's switches and `env`"""
        import inr_mi355x as M
        from inr_mi355x import _lib as L
        kw = dict(dist=self.dist) if self.mfn else {}
        with D._env(**{**D.route_env(self.case), **env}):
            if self.case.route == 1:
                eng.forward(self.x, encB, save=True, **kw)
                g = eng.backward(self.x, encB, self.dout if self.mfn else self.dout[0].contiguous(), **kw)
            else:
                eng.train_step(self.x, encB, self.gt, M.LossSpec(L.LOSS_L2_HALF), count=self.o.count, mask=self.mask, **kw)
                g = eng.grads
            return g.detach().cpu().clone()


def _landed(p, o, case):
    """the build and the route the case is here for, from the plan"""
    s, eng = p.shape, p.engine
    assert eng.step_save_by_tile and eng.tile_rows == s.TL
    with D._env(**D.route_env(case)):
        info = D.step_info(eng, o.B)
        assert info.hidden_blocks == int(s.build[2:]) and (3 if info.hidden_blocks == 12 else 4) == s.WB
        assert bool(info.row_split) == (case.route == 3)
        if case.route == 3:
            w = D.step_split(eng, o.B)
            assert w[0] == 1 and w[11] > 0 and len(o.launches) == 2 and o.launches[1].tile0 == w[11]
        nt, nb = eng.launch_dims(o.B)
        assert eng.workspace(o.B)[1] >= nb + sum(l.chunks for l in o.launches)
        if case.B == "grid":
            assert nt > nb and (case.route == 1 or o.launches[-1].tile0 > 0)
    if case.B == "ragged":
        a = o.launches[0]
        assert a.chunks >= 2 and (a.tile1 - a.tile0) % a.tpc != 0
    if s.split_kernel and case.route != 3:   # one slot, or chunks of 1024 coordinates: square tiles; otherwise half-height
        assert o.launches[0].wbm == (4 if case.B in ("1", "TL-1", "TL", "wbm4") else 2)
    assert all(l.wbm in ((2, 4) if s.split_kernel else (s.WB,)) for l in o.launches)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("case", D.CASES, ids=[c.id for c in D.CASES])
def test_dw_gemm_elementwise(dev, case):
    from conftest import record_parity
    p = D.prepare(case.shape)
    o = D.operands(p, case)
    eng = _bound(p, dev)
    _landed(p, o, case)
    d = _Device(p, o, case, dev)
    got = {}
    if p.shape.split_kernel:
        got["split"] = d.run(eng, p.encB_dev)
        assert torch.equal(_bits(d.run(eng, p.encB_dev)), _bits(got["split"]))
        placed_off = d.run(eng, p.encB_dev, INR_DW_PLACE="0")
        assert torch.equal(_bits(placed_off), _bits(got["split"])), "placement moves workgroups, never a bit"
    with _fp32_kernel():
        got["f32"] = d.run(eng, p.encB_dev)
        assert torch.equal(_bits(d.run(eng, p.encB_dev)), _bits(got["f32"]))
    if p.shape.split_kernel and case.pattern == "dense" and o.B > p.engine.tile_rows:
        assert not torch.equal(got["split"], got["f32"]), "INR_DW_SPLIT selects another kernel"
    for g in got.values():
        assert bool(torch.isfinite(g).all())
    if case.pattern == "onehot" and case.route == 1:
        # every other coordinate adds an exact zero, wherever the chunking puts the sampled one: the covered entries are,
        # to the bit, those of the sampled coordinate alone in a batch of one row
        alone = D.Operands()
        alone.__dict__.update(o.__dict__)
        alone.B, alone.x, alone.dout = 1, o.x[o.row:o.row + 1], o.dout[:, o.row:o.row + 1]
        alone.dist = None if o.dist is None else o.dist[o.row:o.row + 1]
        d1 = _Device(p, alone, case, dev)
        cov = torch.cat([r.idx for r in D.reference(p, alone, torch.float32)])
        for k, g in got.items():
            g1 = d1.run(eng, p.encB_dev, INR_DW_SPLIT=None if k == "split" else "0")
            assert torch.equal(_bits(g1[cov]), _bits(g[cov])), (case.id, k, "a term was dropped, doubled or misplaced")
    r64, r32 = D.reference(p, o, torch.float64), D.reference(p, o, torch.float32)
    failures = []
    for a, (ref_w, ref_b) in zip(r64, D.yardstick(p, o, case, r64, r32)):
        e = {}
        for k, g in got.items():
            ew, eb, zeros_ok = D.err(g, a)
            assert zeros_ok, (case.id, a.name, k, "S == 0 must give an exact zero")
            e[k] = (ew, eb)
        if case.pattern == "allzero":
            assert all(not bool(g[a.idx].any()) for g in got.values())
            continue
        record_parity("dw_gemm:" + case.id, layer=a.name, e_ref_w=ref_w, e_ref_b=ref_b,
                      **{f"e_{k}_{n}": v for k, (ew, eb) in e.items() for n, v in (("w", ew), ("b", eb))})
        print(f"dw_gemm:{case.id} {a.name}: e_ref {ref_w:.3e} {ref_b:.3e} " +
              " ".join(f"{k} {ew:.3e} {eb:.3e}" for k, (ew, eb) in e.items()))
        for k, (ew, eb) in e.items():
            if not ew <= D.FACTOR * ref_w:
                failures.append((a.name, k, "dW", ew, ref_w))
            if not eb <= D.FACTOR * ref_b + D.db_allowance(case):
                failures.append((a.name, k, "db", eb, ref_b))
        if "split" in e:
            for n, es, ef in (("dW", e["split"][0], e["f32"][0]), ("db", e["split"][1], e["f32"][1])):
                if not es <= D.SPLIT_FACTOR * ef:
                    failures.append((a.name, "split vs f32", n, es, ef))
    assert not failures, (case.id, failures)


@pytest.mark.parametrize("shape", ["siren256", "siren300", "wire200"])
def test_stale_workspace(dev, shape):
    """One engine runs a dense step at the `grid` batch with large gradients, then a step at B = 1 and at the batch with a
    ragged last chunk: bitwise the gradients of a fresh engine given the same small batch -- nothing of the large step's
    stash or chunk slabs is read.  (No batch leaves a chunk without tiles: inr_layout.hip chunk_tiles, held by the host test.)"""
    p = D.prepare(shape)
    eng = _bound(p, dev)
    big = D.Case(shape, 2, "grid")
    ob = D.operands(p, big)
    ob.gt = ob.gt * 1e3
    _Device(p, ob, big, dev).run(eng, p.encB_dev)
    fresh_p = MC.prepare(p.shape.mc)
    fresh_p.engine.bind(p.model._flat.detach().clone().to(dev))
    for b in ("1", "ragged"):
        for route in (1, 2):
            case = D.Case(shape, route, b)
            o = D.operands(p, case)
            d = _Device(p, o, case, dev)
            used = d.run(eng, p.encB_dev)
            fresh = d.run(fresh_p.engine, p.encB_dev)
            assert bool(used.any()) and torch.equal(_bits(used), _bits(fresh)), (shape, b, route)
