"""Parity tests proper (``-m gpu``): the HIP path, called through the C-ABI, against
(a) the golden vectors generated from the reference and (b) the CPU oracle on seeded inputs.

Tolerances: the path is fp32 end to end (exact-fp32 MFMA FMA chains); BASELINE.json asks for 1e-5
relative.  Outputs / losses are held to rtol 1e-5 (+ a 1e-6 absolute floor for values near 0);
gradients to 1e-4 element-wise (they are sums of O(B) terms whose order differs from ATen's) and
1e-5 in relative L2 norm.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402  (checker only)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
META = json.load(open(os.path.join(GOLD, "model_meta.json")))


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _load(name):
    return dict(np.load(os.path.join(GOLD, name)))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_library_is_the_hip_build():
    from inr_mi355x import _lib
    lib = _lib.load()
    assert lib.inr_abi_version() == _lib.ABI_VERSION


def test_encoder_and_sincos_accuracy(dev):
    """inr_encode_gauss == Positional_Encoder.embedding (networks.py:30-33); also pins the sincos of the STAND-ALONE
    encoder kernel, which is OCML's sincosf (csrc/inr_encode.hip): abs error vs float64 <= 3e-7 up to |phase| ~ 250 rad.
    (The branch-free sincos_cw inside the fused kernels is held by tests/test_gpu_sincos.py.)"""
    from inr_mi355x import encode_gauss
    g = torch.Generator().manual_seed(0)
    coords = torch.rand(4096, 3, generator=g) * 2 - 1
    B = torch.randn(256, 3, generator=g) * 4
    ref32 = O.encode(coords, B, "gauss")
    out = encode_gauss(coords.to(dev), B.to(dev)).cpu()
    p64 = (2 * np.pi * coords.double().float().double()) @ B.double().t()  # phases as fp32 would round x
    assert float(p64.abs().max()) > 100
    torch.testing.assert_close(out, ref32, rtol=0, atol=2e-5)  # fp32 phase rounding differs (ulp(128)=1.5e-5)
    # accuracy of sincos itself: recompute the fp32 phase exactly as the kernel does, compare in float64
    two_pi = np.float32(6.283185307179586)
    xs = (coords.numpy().astype(np.float32) * two_pi).astype(np.float32)
    Bn = B.numpy().astype(np.float32)
    ph = np.empty((coords.shape[0], 256), dtype=np.float32)
    for s in range(256):
        acc = (xs[:, 0] * Bn[s, 0]).astype(np.float32)
        acc = np.float32(1) * (xs[:, 1].astype(np.float64) * Bn[s, 1] + acc.astype(np.float64)).astype(np.float32)
        acc = (xs[:, 2].astype(np.float64) * Bn[s, 2] + acc.astype(np.float64)).astype(np.float32)
        ph[:, s] = acc
    err_s = np.abs(out[:, :256].numpy().astype(np.float64) - np.sin(ph.astype(np.float64))).max()
    err_c = np.abs(out[:, 256:].numpy().astype(np.float64) - np.cos(ph.astype(np.float64))).max()
    assert err_s <= 3e-7 and err_c <= 3e-7, (err_s, err_c)


def test_logf_encoder_sincos_accuracy(dev):
    """inr_encode_logf (csrc/inr_encode.hip, OCML sincosf) element by element against float64.  Bands are powers of two,
    2^0 .. 2^7, so the kernel's phase fl(fl(2 pi) x_a) * band is exact and numpy restates it to the bit; |phase| reaches
    2^7 * 2 pi = 804 rad.  Bound: the 3e-7 that test_encoder_and_sincos_accuracy holds the gauss encoder's sincosf to.
    Rows: random coordinates, then 0, +-1, +-1/2 and their fp32 neighbours (phases next to multiples of pi)."""
    from inr_mi355x.engine import encode_logf
    g = torch.Generator().manual_seed(3)
    one, half = np.float32(1), np.float32(0.5)
    edge = np.array([0.0, 1.0, np.nextafter(one, np.float32(0)), 0.5, np.nextafter(half, np.float32(0)),
                     np.nextafter(half, one), 0.25, 0.75], dtype=np.float32)
    edge = np.concatenate([edge, -edge])
    coords = torch.cat([torch.rand(1000, 3, generator=g) * 2 - 1, torch.from_numpy(np.repeat(edge[:, None], 3, axis=1))])
    bands = 2.0 ** torch.arange(8, dtype=torch.float32)
    nb = bands.numel()
    out = encode_logf(coords.to(dev), bands.reshape(-1, 1).to(dev)).cpu().numpy().astype(np.float64)
    assert out.shape == (coords.shape[0], 6 * nb)
    xs = (np.float32(6.283185307179586) * coords.numpy()).astype(np.float32)
    worst = 0.0
    for a in range(3):
        ph = (xs[:, a:a + 1] * bands.numpy()[None, :]).astype(np.float32).astype(np.float64)  # exact: a power of two
        assert float(np.abs(ph).max()) > 800
        blk = out[:, a * 2 * nb:(a + 1) * 2 * nb]
        worst = max(worst, float(np.abs(blk[:, :nb] - np.sin(ph)).max()), float(np.abs(blk[:, nb:] - np.cos(ph)).max()))
    print("logf sincosf max abs error", worst)
    assert worst <= 3e-7, worst


@pytest.mark.parametrize("name", ["SIREN", "SIREN_tanh", "SIREN_raw3", "FFN"])
def test_tier1_golden(dev, name):
    """Drop-in class + stock torch.optim.Adam (tier 1) reproduce the reference's forward, loss,
    gradients and parameters after 1 and 3 Adam steps (with and without weight decay)."""
    import inr_mi355x as M
    meta = META[name]
    arrs = _load(f"model_{name}.npz")
    cls = {"SIREN": M.SIREN, "FFN": M.FFN}[meta["model"]]
    x, gt = _t(arrs["x"]).to(dev), _t(arrs["gt"]).to(dev)
    for wd_tag, wd in (("wd0", 0.0), ("wd1", meta["wd1"])):
        torch.manual_seed(meta["seed"])
        if meta["encoder"] is not None:
            enc = M.Positional_Encoder(meta["encoder"], device=dev)
            assert torch.equal(enc.B.cpu(), _t(arrs["enc_B"]))
        model = cls(meta["net"])
        sd = model.state_dict()
        gold_keys = [k[3:] for k in arrs if k.startswith("sd/")]
        assert list(sd.keys()) == gold_keys
        for k in gold_keys:  # bit-exact initialisation
            assert torch.equal(sd[k], _t(arrs["sd/" + k])), k
        model = model.to(dev)
        optim = torch.optim.Adam(model.parameters(), lr=meta["lr"], betas=(0.9, 0.999), weight_decay=wd)
        for step in range(1, 4):
            out = model(x)
            optim.zero_grad()
            loss = 0.5 * torch.nn.functional.mse_loss(out, gt)
            loss.backward()
            if step == 1 and wd_tag == "wd0":
                torch.testing.assert_close(out.detach().cpu(), _t(arrs["out"]), rtol=1e-5, atol=1e-6)
                torch.testing.assert_close(loss.detach().cpu(), _t(arrs["loss"]), rtol=1e-5, atol=0)
                for k, p in model.named_parameters():
                    ref = _t(arrs["grad/" + k])
                    torch.testing.assert_close(p.grad.cpu(), ref, rtol=1e-4, atol=1e-7, msg=lambda m: f"{k}: {m}")
                    assert rel_l2(p.grad.cpu(), ref) < 1e-5, k
            optim.step()
            if step in (1, 3):
                for k, v in model.state_dict().items():
                    ref = _t(arrs[f"{wd_tag}/step{step}/" + k])
                    torch.testing.assert_close(v.cpu(), ref, rtol=1e-5, atol=2e-6,
                                               msg=lambda m: f"{wd_tag} step{step} {k}: {m}")


@pytest.mark.parametrize("name", ["SIREN", "SIREN_tanh", "FFN"])
def test_tier2_fused_golden(dev, name):
    """Fused train_step (encoder fused into layer 0) + inr_adam_step (tier 2) give the same
    parameters as the reference after 1 and 3 steps."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    meta = META[name]
    arrs = _load(f"model_{name}.npz")
    cls = {"SIREN": M.SIREN, "FFN": M.FFN}[meta["model"]]
    coords, gt = _t(arrs["coords"]).to(dev), _t(arrs["gt"]).to(dev)
    for wd_tag, wd in (("wd0", 0.0), ("wd1", meta["wd1"])):
        torch.manual_seed(meta["seed"])
        enc = M.Positional_Encoder(meta["encoder"], device=dev)
        model = cls(meta["net"]).to(dev)
        eng = model.fused_engine(meta["encoder"]["embedding_size"])
        spec = M.LossSpec(L.LOSS_L2_HALF)
        for step in range(1, 4):
            loss = eng.train_step(coords, enc.B.contiguous(), gt, spec)
            if step == 1 and wd_tag == "wd0":
                torch.testing.assert_close(loss.cpu(), _t(arrs["loss"]), rtol=1e-5, atol=0)
                flat = eng.grads.cpu()
                for (off, n, shp, _c), (k, _) in zip(model._layout, model.named_parameters()):
                    ref = _t(arrs["grad/" + k])
                    torch.testing.assert_close(flat[off:off + n].view(shp), ref, rtol=1e-4, atol=1e-7,
                                               msg=lambda m: f"{k}: {m}")
            eng.adam_step(meta["lr"], 0.9, 0.999, 1e-8, wd)
            if step in (1, 3):
                for k, v in model.state_dict().items():
                    ref = _t(arrs[f"{wd_tag}/step{step}/" + k])
                    torch.testing.assert_close(v.cpu(), ref, rtol=1e-5, atol=2e-6,
                                               msg=lambda m: f"{wd_tag} step{step} {k}: {m}")


FULL_NET = dict(network_input_size=512, network_output_size=2, network_depth=5, network_width=256, last_tanh=True)
FULL_ENC = dict(embedding="gauss", scale=4, embedding_size=256, coordinates_size=3)


def _oracle_grads(sd, B_enc, coords, gt, net, mask=None):
    keys = list(sd.keys())
    params = {k: sd[k].clone().requires_grad_(True) for k in keys}
    out = O.siren_forward(params, O.encode(coords, B_enc, "gauss"), net)
    o, g = (out, gt) if mask is None else (out[mask], gt[mask])
    loss = O.loss_l2_half(o, g)
    grads = torch.autograd.grad(loss, list(params.values()))
    return out.detach(), loss.detach(), torch.cat([x.reshape(-1) for x in grads])


@pytest.mark.parametrize("B", [1, 127, 128, 129, 1000, 4133])
def test_full_size_siren_vs_oracle(dev, B):
    """SIREN 5x256 / gauss-512 (the graded shape), ragged batch sizes, masked rows."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    torch.manual_seed(0)
    enc = M.Positional_Encoder(FULL_ENC, device=dev)
    model = M.SIREN(FULL_NET)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    g = torch.Generator().manual_seed(B)
    coords = torch.rand(B, 3, generator=g) * 2 - 1
    gt = torch.randn(B, 2, generator=g) * 0.2
    mask = torch.rand(B, generator=g) < 0.6 if B > 100 else None
    ref_out, ref_loss, ref_grad = _oracle_grads(sd, enc.B.cpu(), coords, gt, FULL_NET, mask)
    eng = model.fused_engine(256)
    out = eng.forward(coords.to(dev), enc.B.contiguous(), save=False).cpu()
    torch.testing.assert_close(out, ref_out, rtol=1e-5, atol=2e-6)
    assert rel_l2(out, ref_out) < 1e-5
    cnt = B if mask is None else int(mask.sum())
    m = None if mask is None else mask.to(torch.uint8).to(dev)
    loss = eng.train_step(coords.to(dev), enc.B.contiguous(), gt.to(dev), M.LossSpec(L.LOSS_L2_HALF), count=cnt, mask=m)
    torch.testing.assert_close(loss.cpu(), ref_loss, rtol=1e-5, atol=0)
    got = eng.grads.cpu()
    assert rel_l2(got, ref_grad) < 1e-5
    torch.testing.assert_close(got, ref_grad, rtol=1e-3, atol=float(ref_grad.abs().max()) * 1e-5)
    # tier-1 path (materialised encoding, separate forward / backward kernels) agrees too
    x = enc.embedding(coords.to(dev))
    o1 = model(x)
    l1 = 0.5 * torch.nn.functional.mse_loss(o1 if mask is None else o1[mask.to(dev)],
                                            gt.to(dev) if mask is None else gt.to(dev)[mask.to(dev)])
    l1.backward()
    g1 = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu()
    assert rel_l2(o1.detach().cpu(), ref_out) < 1e-5
    assert rel_l2(g1, ref_grad) < 1e-5


def test_persistent_blocks_and_determinism(dev):
    """B > 256 tiles: blocks loop over tiles and continue their slab sums; two runs are bitwise equal."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    torch.manual_seed(1)
    enc = M.Positional_Encoder(FULL_ENC, device=dev)
    model = M.SIREN(FULL_NET)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    B = 256 * 128 + 777
    g = torch.Generator().manual_seed(5)
    coords = torch.rand(B, 3, generator=g) * 2 - 1
    gt = torch.randn(B, 2, generator=g) * 0.2
    eng = model.fused_engine(256)
    spec = M.LossSpec(L.LOSS_L2_HALF)
    l_a = eng.train_step(coords.to(dev), enc.B.contiguous(), gt.to(dev), spec).clone()
    g_a = eng.grads.clone()
    l_b = eng.train_step(coords.to(dev), enc.B.contiguous(), gt.to(dev), spec).clone()
    assert torch.equal(g_a, eng.grads) and torch.equal(l_a, l_b)
    _, ref_loss, ref_grad = _oracle_grads(sd, enc.B.cpu(), coords, gt, FULL_NET)
    torch.testing.assert_close(l_a.cpu(), ref_loss, rtol=1e-5, atol=0)
    assert rel_l2(g_a.cpu(), ref_grad) < 1e-5


@pytest.mark.parametrize("kind", ["L1", "tanh", "LogSpace", "HDR", "MSLE"])
def test_losses_fused_and_tier1(dev, kind):
    """Pointwise losses: fused in-kernel evaluation and inr_loss_grad agree with the oracle's autograd."""
    import inr_mi355x as M
    meta = META["SIREN"]
    arrs = _load("model_SIREN.npz")
    opts = dict(hdr_eps=1e-3, hdr_ff_sigma=2, hdr_ff_factor=0.5)
    torch.manual_seed(meta["seed"])
    enc = M.Positional_Encoder(meta["encoder"], device=dev)
    model = M.SIREN(meta["net"])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    coords, gt = _t(arrs["coords"]), _t(arrs["gt"])
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = O.siren_forward(params, O.encode(coords, enc.B.cpu(), "gauss"), meta["net"])
    f = torch.exp(-(coords[:, 1] ** 2 + coords[:, 2] ** 2) / (2 * 2.0 ** 2))
    A = float(torch.mean((1 - f) ** 2))
    loss = {"L1": lambda: O.loss_l1_half(out, gt), "tanh": lambda: O.loss_tanh(out, gt)[0],
            "LogSpace": lambda: O.loss_logspace(out, gt, opts), "HDR": lambda: O.loss_hdr(out, gt, coords, opts)[0],
            "MSLE": lambda: 0.5 * O.loss_msle(out, gt)}[kind]()
    ref_grad = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(params.values()), retain_graph=True)])
    (ref_dout,) = torch.autograd.grad(loss, out)
    spec = M.LossSpec.from_config({"loss": kind, "loss_opts": opts})
    eng = model.fused_engine(8)
    l = eng.train_step(coords.to(dev), enc.B.contiguous(), gt.to(dev), spec, hdr_A=A)
    torch.testing.assert_close(l.cpu(), loss.detach(), rtol=2e-5, atol=0)
    assert rel_l2(eng.grads.cpu(), ref_grad) < 2e-5
    l2, dout = eng.loss_grad(spec, out.detach().to(dev).contiguous(), gt.to(dev), count=coords.shape[0], hdr_A=A)
    torch.testing.assert_close(l2.cpu(), loss.detach(), rtol=2e-5, atol=0)
    torch.testing.assert_close(dout.cpu(), ref_dout, rtol=1e-4, atol=1e-9)


def test_trajectory_golden(dev):
    """The trainer (sequential batches, per-epoch LambdaLR, fused steps) tracks the trajectory the
    reference's classes produced under the train.py loop."""
    from inr_mi355x.train import INRTrainer
    arrs = _load("trajectory.npz")
    meta = json.load(open(os.path.join(GOLD, "trajectory_meta.json")))
    coords, image = _t(arrs["coords"]), _t(arrs["image"])
    # plain | + Regularization_L1 + weight decay | + Regularization_L2 | CenterLoss ('LSL': forward -> pointwise part ->
    # two bands of torch.randperm pairs -> backward; the trainer draws from the generator its constructor seeded)
    for tag in ("SIREN_L2", "SIREN_L2_reg", "SIREN_regL2", "SIREN_LSL"):
        cfg = meta["cases"][tag]
        tr = INRTrainer(cfg, image, coords, tuple(meta["shape"]), dev, seed=meta["seed"])
        got = [s[1] for s in tr.fit(meta["steps"], log_every=1)]
        ref = arrs[tag + "/losses"]
        # (SIREN_L2_reg: the logged loss of the reference includes the L1 penalty value, train.py:185-192)
        np.testing.assert_allclose(np.array(got), ref, rtol=2e-4, err_msg=tag)
        out = tr.predict_all().cpu()
        torch.testing.assert_close(out, _t(arrs[tag + "/final_out"]), rtol=1e-3, atol=2e-5, msg=lambda m: f"{tag}: {m}")
        for k, v in tr.model.state_dict().items():
            torch.testing.assert_close(v.cpu(), _t(arrs[f"{tag}/final_sd/{k}"]), rtol=1e-4, atol=2e-6,
                                       msg=lambda m: f"{tag} {k}: {m}")


def test_device_resident_adam_and_graph_steps(dev):
    """(i) inr_adam_step_dev (step count + bias corrections read from device memory) leaves bit-identical parameters,
    moments and packed weights to inr_adam_step; (ii) a fit whose steps are replayed HIP graphs (one per batch of
    the epoch, captured on first use; the per-epoch learning-rate change is a new table, not a new graph; a short last
    batch; L1 penalty + weight decay inside the Adam kernel) is bit-identical to the same fit launched eagerly."""
    import inr_mi355x as M
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    net = dict(network_input_size=64, network_output_size=2, network_depth=3, network_width=64)
    engs = []
    for _ in range(2):
        torch.manual_seed(5)
        engs.append(M.SIREN(net).to(dev)._engine())
    g = torch.Generator().manual_seed(1)
    for t in range(1, 8):
        grad = torch.randn(engs[0].n_params, generator=g).to(dev) * 1e-3
        for e in engs:
            e.grads.copy_(grad)
        lr = 1e-3 if t < 5 else 7e-4
        engs[0].adam_step(lr, 0.9, 0.999, 1e-8, 1e-4, 1e-6, 0.0)
        if t == 3:  # an eager step in between moves the host count only: the device copy is refreshed
            engs[1].adam_step(lr, 0.9, 0.999, 1e-8, 1e-4, 1e-6, 0.0)
        else:
            engs[1].adam_step_dev(lr, 0.9, 0.999, 1e-8, 1e-4, 1e-6, 0.0)
        for name in ("params", "exp_avg", "exp_avg_sq", "packed"):
            assert torch.equal(getattr(engs[0], name), getattr(engs[1], name)), (t, name)
    assert int(engs[1]._step_dev) == engs[1].step == 7

    image, kc, shape = make_kspace(2, 16, 12)  # 384 rows: batches of 150, 150, 84
    enc = dict(embedding="gauss", scale=2, embedding_size=32, coordinates_size=3)
    for extra in (dict(), dict(loss="HDR", loss_opts=dict(hdr_eps=1e-2, hdr_ff_sigma=1.0, hdr_ff_factor=0.1)),
                  dict(regularization=dict(type="L1", strenght=1e-6), weight_decay=1e-5)):
        cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=150, max_epoch=3, weight_decay=0.0, beta1=0.9,
                   beta2=0.999, net=net, encoder=enc)
        cfg.update(extra)
        fits = []
        for graph in (False, True):
            tr = INRTrainer(cfg, image, kc, shape, dev, seed=3, graph_steps=graph)
            assert tr.graph_steps == graph
            if graph and not extra:
                tr.prepare_graphs()
            losses = [s[1] for s in tr.fit(8, log_every=1)]  # 2 2/3 epochs: every graph replayed, two lr changes
            fits.append((losses, tr.engine.params.clone(), tr.engine.exp_avg_sq.clone()))
            if graph:
                assert len(tr._graphs) == 3 and tr.engine.step == 8
        assert fits[0][0] == fits[1][0], extra
        assert torch.equal(fits[0][1], fits[1][1]) and torch.equal(fits[0][2], fits[1][2]), extra


@pytest.mark.parametrize("model,B", [("SIREN", 40000), ("WIRE", 25000), ("SIREN512", 20000)])
def test_split_step_overlap_matches_plain_schedule(dev, model, B):
    """Batches whose tiles do not fill the last round of the persistent grid (SIREN 5x256: 313 tiles of 128 rows =
    256 + 57; WIRE: 391 tiles of 64 = 256 + 135; SIREN 8x512: 313 tiles of 64) run as a split step: the weight-gradient
    GEMM of the finished tiles on a side stream beside the fused kernel's partial round (inr_layout.hip, step_schedule).
    Same forward, same per-tile sums, another chunking of the GEMM: loss and last-layer gradients bit-identical to
    the plain schedule (INR_OVERLAP=0), the GEMM's layers to summation order; run-to-run deterministic; and the
    workspace the plan asks for covers both schedules."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    torch.manual_seed(0)
    if model == "SIREN":
        enc = M.Positional_Encoder(FULL_ENC, device=dev)
        eng = M.SIREN(FULL_NET).to(dev).fused_engine(256)
        enc_B = enc.B.contiguous()
    elif model == "SIREN512":
        enc = M.Positional_Encoder(FULL_ENC, device=dev)
        eng = M.SIREN(dict(FULL_NET, network_depth=4, network_width=512)).to(dev).fused_engine(256)
        enc_B = enc.B.contiguous()
    else:
        eng = M.WIRE(dict(network_input_size=3, network_output_size=2, network_depth=4, network_width=256,
                          first_omega_0=30, hidden_omega_0=30, scale=15)).to(dev)._engine()
        enc_B = None
    g = torch.Generator().manual_seed(7)
    coords = (torch.rand(B, 3, generator=g) * 2 - 1).to(dev)
    gt = (torch.randn(B, 2, generator=g) * 0.2).to(dev)
    spec = M.LossSpec(L.LOSS_L2_HALF)
    nt, nb = eng.launch_dims(B)
    assert nt > nb and nt % nb != 0

    def step():
        l = float(eng.train_step(coords, enc_B, gt, spec))
        torch.cuda.synchronize()
        return l, eng.grads.clone()

    old = os.environ.get("INR_OVERLAP")
    try:
        os.environ["INR_OVERLAP"] = "0"
        slabs_plain = eng.workspace(B)[1]
        l0, g0 = step()
        os.environ["INR_OVERLAP"] = "1"
        slabs_split = eng.workspace(B)[1]
        l1, g1 = step()
        l2, g2 = step()
    finally:
        if old is None:
            os.environ.pop("INR_OVERLAP", None)
        else:
            os.environ["INR_OVERLAP"] = old
    assert slabs_split > slabs_plain  # the split schedule is in use: part A's chunks come on top
    assert l0 == l1 == l2
    if model == "SIREN":  # the fork into the side stream and the join are captured with the rest of the step
        p0, m0 = eng.params.clone(), (eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.step)
        sg = eng.capture_step(lambda: eng.train_step(coords, enc_B, gt, spec), 1e-4)
        sg.replay(1e-4)
        torch.cuda.synchronize()
        assert torch.equal(eng.grads, g1)
        p_graph = eng.params.clone()
        eng.params.copy_(p0); eng.exp_avg.copy_(m0[0]); eng.exp_avg_sq.copy_(m0[1]); eng.step = m0[2]
        eng.pack()
        eng.train_step(coords, enc_B, gt, spec)
        eng.adam_step(1e-4)
        assert torch.equal(eng.params, p_graph)
        eng.params.copy_(p0); eng.exp_avg.copy_(m0[0]); eng.exp_avg_sq.copy_(m0[1]); eng.step = m0[2]
        eng.pack()
    assert torch.equal(g1, g2)
    assert rel_l2(g1, g0) < 2e-6
    n_last = eng.out_features * (eng.desc.width + 1) if model != "WIRE" else 0
    if n_last:  # the last layer's dW / db never pass through the GEMM: same sums, same order
        assert torch.equal(g1[-n_last:], g0[-n_last:])


@pytest.mark.parametrize("case", ["siren", "siren_reg", "siren_bf16", "wire", "siren_mask"])
def test_one_call_step_matches_two_calls(dev, case):
    """inr_train_adam_step (the Adam update inside the slab reduction's launch; two launches behind the same entry for
    plans whose slabs do not have the flat layout, e.g. WIRE) against inr_train_step + inr_adam_step: parameters,
    moments, packed images and logged losses bit-identical over eight steps with two learning-rate changes."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, kc, shape = make_kspace(2, 16, 12)  # 384 rows: batches of 150, 150, 84
    enc = dict(embedding="gauss", scale=2, embedding_size=32, coordinates_size=3)
    cfg = dict(model="SIREN", loss="L2", lr=1e-3, batch_size=150, max_epoch=3, weight_decay=0.0, beta1=0.9, beta2=0.999,
               net=dict(network_input_size=64, network_output_size=2, network_depth=3, network_width=64), encoder=enc)
    if case == "siren_reg":
        cfg.update(regularization=dict(type="L1", strenght=1e-6), weight_decay=1e-5)
    if case == "siren_bf16":
        cfg.update(precision="bf16", net=dict(network_input_size=64, network_output_size=2, network_depth=4,
                                              network_width=256, last_tanh=True))
    if case == "siren_mask":
        cfg.update(undersampling="grid-2*1", loss="HDR", loss_opts=dict(hdr_eps=1e-2, hdr_ff_sigma=1.0, hdr_ff_factor=0.1))
    if case == "wire":
        cfg.update(model="WIRE", encoder=dict(embedding="none", scale=1, embedding_size=3, coordinates_size=3),
                   net=dict(network_input_size=3, network_output_size=2, network_depth=2, network_width=64,
                            first_omega_0=10, hidden_omega_0=10, scale=5))
    fits, old = [], os.environ.get("INR_ONE_CALL_STEPS")
    try:
        for flag in ("0", "1"):
            os.environ["INR_ONE_CALL_STEPS"] = flag
            tr = INRTrainer(cfg, image, kc, shape, dev, seed=3)
            assert tr.one_call_steps == (flag == "1")
            losses = [s_[1] for s_ in tr.fit(8, log_every=1)]
            e = tr.engine
            fits.append((losses, e.params.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(), e.packed.clone(), e.grads.clone()))
            assert e.step == 8
    finally:
        if old is None:
            os.environ.pop("INR_ONE_CALL_STEPS", None)
        else:
            os.environ["INR_ONE_CALL_STEPS"] = old
    assert fits[0][0] == fits[1][0]
    for a, b in zip(fits[0][1:], fits[1][1:]):
        assert torch.equal(a, b)


def test_center_loss_vs_reference_vectors(dev):
    """CenterLoss through inr_loss_grad(INR_LOSS_CENTER) + inr_center_pairs_grad against value and gradient of the
    reference class (tests/golden/center.npz, pairs from torch.randperm under the fixture's seed)."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    from inr_mi355x.train import center_pair_rows
    arrs = _load("center.npz")
    out, gt, kc = (_t(arrs[k]).to(dev).contiguous() for k in ("out", "gt", "kcoords"))
    net = dict(network_input_size=3, network_output_size=2, network_depth=2, network_width=32)
    eng = M.SIREN(net).to(dev)._engine()  # (any engine: the loss entry points only use its scalar buffer and stream)
    f = torch.exp(-(kc[:, 1] ** 2 + kc[:, 2] ** 2) / (2 * 2.0 ** 2))
    A = float(torch.mean((1 - f) ** 2))
    for tag, ms in (("ms50", 50), ("ms3000", 3000)):
        spec = M.LossSpec(L.LOSS_CENTER, 1e-3, 2.0, 0.5, ms)
        loss, dout = eng.loss_grad(spec, out, gt, out.shape[0], hdr_A=A)
        torch.manual_seed(int(arrs["seed"]))
        n_bands = 0
        for rows_a, rows_b in center_pair_rows(kc, ms):
            loss = eng.center_pairs_grad(out, gt, dout, rows_a, rows_b, 0.1)
            n_bands += 1
        assert n_bands == 2
        torch.testing.assert_close(loss.cpu().reshape(1), _t(arrs[tag + "/loss"]), rtol=1e-5, atol=0)
        torch.testing.assert_close(dout.cpu(), _t(arrs[tag + "/grad"]), rtol=1e-4, atol=1e-8)
    # malformed calls are refused, rows outside the batch ignored
    bad = torch.tensor([0, 10 ** 9], device=dev)
    eng.center_pairs_grad(out, gt, dout, bad, bad.flip(0).contiguous(), 0.1)
    torch.cuda.synchronize()


def test_eval_chain_and_psnr(dev):
    """Round trip at BASELINE shape: fitting-free property -- reconstructing the ground truth k-space
    gives PSNR -> +inf side (> 60 dB) and the device chain equals the oracle's CPU chain."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.evalchain import reconstruct, psnr
    image, coords, shape = make_kspace(4, 64, 48, seed=3)
    ref = O.reconstruct(image, shape, False)
    got = reconstruct(image.to(dev), shape, False).cpu()
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-6)
    noisy = image + 1e-3 * torch.randn_like(image)
    p_dev = float(psnr(reconstruct(image.to(dev), shape, False), reconstruct(noisy.to(dev), shape, False)))
    p_cpu = float(O.psnr(ref, O.reconstruct(noisy, shape, False)))
    assert abs(p_dev - p_cpu) < 1e-2


def test_logf_encoder_and_trainer(dev):
    """Positional_Encoder 'LogF' (networks.py:16,24-29) through inr_encode_logf, and a SIREN fit on it
    (unfused first layer: the [B,6*nb] features are materialised, as the reference does)."""
    import inr_mi355x as M
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    cfgE = dict(embedding="LogF", scale=5, embedding_size=60, coordinates_size=3)
    enc = M.Positional_Encoder(cfgE, device=dev)
    assert enc.B.shape == (10, 1)
    g = torch.Generator().manual_seed(0)
    coords = torch.rand(3001, 3, generator=g) * 2 - 1
    ref = O.encode(coords, enc.B.cpu(), "LogF")
    got = enc.embedding(coords.to(dev)).cpu()
    assert got.shape == (3001, 60)
    torch.testing.assert_close(got, ref, rtol=0, atol=1e-5)  # phases up to 2 pi 32 ~ 200 rad: ulp(200) = 1.5e-5
    image, kc, shape = make_kspace(2, 16, 12)
    cfg = dict(model="SIREN", loss="L2", lr=1e-4, batch_size=150, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999,
               net=dict(network_input_size=60, network_output_size=2, network_depth=3, network_width=32), encoder=cfgE)
    tr = INRTrainer(cfg, image, kc, shape, dev, seed=2)
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    want = O.train_single_scale(cfg, sd, tr.encoder.B.cpu(), kc, image, 5)
    got = np.array([s[1] for s in tr.fit(5, log_every=1)])
    np.testing.assert_allclose(got, np.array(want), rtol=5e-5)


def test_ring_ensemble_vs_oracle_and_rank_independence(dev):
    """One SIREN per k-means ring: every ring's loss curve equals the oracle's single-model loop
    run with that ring's row mask; a rank of a 2-rank job reproduces exactly its rings of the 1-rank job (models
    are independent: no collective in training)."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train_ring_ensemble import RingEnsembleTrainer
    C, H, W = 2, 40, 32
    image, coords, shape = make_kspace(C, H, W)
    # one coil per batch: every ring is present in every batch (an absent ring is a skipped optimizer step in the
    # reference -- grads stay None -- which the single-model oracle loop has no notion of; checked separately below)
    cfg = dict(model="SIREN", loss="L2", lr=2e-4, batch_size=H * W, max_epoch=3, weight_decay=0.0, beta1=0.9,
               beta2=0.999, partition=dict(no_steps=20, no_models=3),
               net=dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32),
               encoder=dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3))
    tr = RingEnsembleTrainer(cfg, image, coords, shape, dev, seed=5)
    assert tr.no_models == 3 and tr.owned == [0, 1, 2] and tr.radii[0] == 0 and tr.radii[-1] == 5
    sds = {i: {k: v.detach().cpu().clone() for k, v in tr.models[i].state_dict().items()} for i in tr.owned}
    logged = tr.fit(5, log_every=1)
    dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
    for i in range(3):
        mask = (dist >= tr.radii[i]) & (dist <= tr.radii[i + 1])
        want = O.train_single_scale(cfg, sds[i], tr.encoder.B.cpu(), coords, image, 5, mask=mask)
        got = [l[1][i] for l in logged]
        np.testing.assert_allclose(np.array(got, dtype=float), np.array(want), rtol=5e-5, err_msg=f"ring {i}")
    rec = tr.predict_all()
    assert rec.shape == (C * H * W, 2) and bool(torch.isfinite(rec).all())
    assert np.isfinite(tr.evaluate())
    # rank 1 of 2 owns ring 1 only and walks the same trajectory
    tr1 = RingEnsembleTrainer(cfg, image, coords, shape, dev, seed=5, rank=1, world=2)
    assert tr1.owned == [1]
    l1 = tr1.fit(5, log_every=1)
    assert [l[1][1] for l in l1] == [l[1][1] for l in logged]
    assert all(l[1][0] is None and l[1][2] is None for l in l1)
    # a batch that misses a ring leaves that ring's model and its Adam state untouched
    tr2 = RingEnsembleTrainer(dict(cfg, batch_size=4 * W), image, coords, shape, dev, seed=5)
    before = tr2.engines[0].params.clone()
    out = tr2.step(0, 0)  # rows y = 0..3: far from the centre
    assert out[0] is None and out[2] is not None
    assert torch.equal(before, tr2.engines[0].params) and tr2.engines[0].step == 0 and tr2.engines[2].step == 1


@pytest.mark.parametrize("model", ["SIREN", "WIRE", "Gabor"])
def test_checkpoint_roundtrip_and_torch_adam_interchange(dev, model, tmp_path):
    """{'net','enc','opt'} (train.py:247-250): (i) save -> new trainer with config['pretrain'] -> continue equals the
    uninterrupted run bit for bit; (ii) the 'opt' entry loads into a stock torch.optim.Adam over the drop-in
    model's parameters, and a checkpoint written from such an optimizer resumes in the fused trainer."""
    import inr_mi355x as M
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(2, 24, 20)
    wire = model == "WIRE"
    net = dict(network_input_size=3 if wire else 32, network_output_size=2, network_depth=2 if wire else 3,
               network_width=32, first_omega_0=10, hidden_omega_0=10, scale=5)
    cfg = dict(model=model, loss="L2", lr=1e-3, batch_size=300, max_epoch=3, weight_decay=0.01, beta1=0.9, beta2=0.999,
               net=net, encoder=dict(embedding="none" if wire else "gauss", scale=2, embedding_size=16,
                                     coordinates_size=3))
    full = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    a = INRTrainer(cfg, image, coords, shape, dev, seed=3)
    l_full = [s[1] for s in full.fit(8, log_every=1)]
    la = [s[1] for s in a.fit(4, log_every=1)]
    path = str(tmp_path / "model_000004.pt")
    torch.save(a.checkpoint(), path)
    b = INRTrainer(dict(cfg, pretrain=path), image, coords, shape, dev, seed=99)  # different init: all from the file
    assert b.engine.step == 4
    b.global_step = 4
    lb = []
    for s in range(4, 8):
        lb.append(float(b.step(s // b.steps_per_epoch, s % b.steps_per_epoch)))
    assert la + lb == l_full
    # (ii) torch.optim.Adam accepts the 'opt' entry
    ck = torch.load(path, map_location=dev)
    m = getattr(M, model, None) or getattr(__import__("inr_mi355x.mfn", fromlist=[model]), model + "Net")
    torch.manual_seed(0)
    mod = m(net).to(dev)
    mod.load_state_dict(ck["net"])
    opt = torch.optim.Adam(mod.parameters(), lr=cfg["lr"], betas=(0.9, 0.999), weight_decay=cfg["weight_decay"])
    opt.load_state_dict(ck["opt"])
    st = opt.state_dict()["state"]
    assert len(st) == len(ck["opt"]["state"]) and all(int(v["step"]) == 4 for v in st.values())
    ck2 = {"net": mod.state_dict(), "enc": ck["enc"], "opt": opt.state_dict()}
    c = INRTrainer(cfg, image, coords, shape, dev, seed=7)
    c.load_checkpoint(ck2)
    assert c.engine.step == 4
    assert float(c.step(4 // c.steps_per_epoch, 4 % c.steps_per_epoch)) == lb[0]


@pytest.mark.parametrize("module,cfg,extra", [
    ("inr_mi355x.train", "config_siren_kspace.yaml", []),
    ("inr_mi355x.train", "config_wire_kspace.yaml", []),
    ("inr_mi355x.train", "config_siren_radial_tv_bf16.yaml", []),
    ("inr_mi355x.train_kspace_multiscale", "config_fourier_multiscale.yaml", []),
])
def test_cli_runs_the_shipped_configs(dev, module, cfg, extra, tmp_path):
    """`python -m inr_mi355x.train --config ...` (the reference's CLI flags, train.py:255-258) on the configs/ that
    mirror the BASELINE workloads, shrunk to a small synthetic k-space and a few steps."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "mri-implicit-neural-representations_amd"))
    out = subprocess.run([sys.executable, "-m", module, "--config", os.path.join(root, "configs", cfg),
                          "--output_path", str(tmp_path), "--synthetic", "2,64,48", "--max_steps", "4"] + extra,
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["steps"] == 4 and np.isfinite(res["psnr"])
    ck = torch.load(os.path.join(str(tmp_path), "model_000004.pt"), map_location="cpu")
    assert set(ck) == {"net", "enc", "opt"}


@pytest.mark.parametrize("module,cfg", [("inr_mi355x.train", "config_siren_kspace.yaml"),
                                        ("inr_mi355x.train_kspace_multiscale", "config_fourier_multiscale.yaml")])
def test_cli_ingests_a_scan_file(dev, module, cfg, tmp_path):
    """Without --synthetic the CLIs read the scan the config names (train.py:271-287): data_root/<data>_multicoil_<set>/,
    entry ``sample``, slice ``slice`` -- here a two-file directory of .npz scans with an ISMRMRD header."""
    import subprocess
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "brain_multicoil_train"
    d.mkdir()
    rng = np.random.default_rng(0)
    hdr = ("<ismrmrdHeader xmlns='http://www.ismrm.org/ISMRMRD'><encoding><reconSpace><matrixSize><x>48</x><y>40</y>"
           "<z>1</z></matrixSize></reconSpace></encoding></ismrmrdHeader>").encode()
    for name in ("file_brain_0.npz", "file_brain_1.npz"):
        ks = (rng.standard_normal((2, 3, 64, 44)) + 1j * rng.standard_normal((2, 3, 64, 44))).astype(np.complex64)
        np.savez(d / name, kspace=ks, ismrmrd_header=np.frombuffer(hdr, np.uint8))
    config = yaml.safe_load(open(os.path.join(root, "configs", cfg)))
    config.update(data="brain", data_root=str(tmp_path), set="train", sample=1, slice=1, batch_size=1000)
    cpath = tmp_path / "cfg.yaml"
    yaml.safe_dump(config, open(cpath, "w"))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "mri-implicit-neural-representations_amd"))
    out = subprocess.run([sys.executable, "-m", module, "--config", str(cpath), "--output_path", str(tmp_path),
                          "--max_steps", "3"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and np.isfinite(res["psnr"])


def test_full_baseline_size_properties(dev):
    """BASELINE config 2 at its real size (640x368x15 = 3 532 800 coordinates, SIREN 5x256, batch 25 000), through
    properties that need no oracle run: (i) gradient additivity -- the fused step on a batch equals the sum of the
    fused steps on a ragged split of it (same global count); (ii) tiling invariance -- the full-grid forward sweep
    does not depend on the chunking; (iii) run-to-run determinism; (iv) PSNR of the fit target against itself."""
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    from inr_mi355x.evalchain import psnr, reconstruct
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(15, 640, 368, seed=1234, normalization="coil")
    assert coords.shape[0] == 3532800
    cfg = dict(model="SIREN", loss="L2", lr=3e-5, batch_size=25000, max_epoch=1000, weight_decay=0.0, beta1=0.9,
               beta2=0.999, net=FULL_NET, encoder=FULL_ENC)
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=0)
    assert tr.steps_per_epoch == 142
    eng, spec = tr.engine, M.LossSpec(L.LOSS_L2_HALF)
    lo, hi, cut = 1_000_000, 1_025_000, 1_010_037
    x, gt = tr.coords, tr.image
    l_all = float(eng.train_step(x[lo:hi], tr.enc_B, gt[lo:hi], spec, count=25000))
    g_all = eng.grads.clone()
    l_a = float(eng.train_step(x[lo:cut], tr.enc_B, gt[lo:cut], spec, count=25000))
    g_a = eng.grads.clone()
    l_b = float(eng.train_step(x[cut:hi], tr.enc_B, gt[cut:hi], spec, count=25000))
    g_sum = g_a + eng.grads
    assert abs(l_a + l_b - l_all) <= 2e-6 * abs(l_all)
    assert rel_l2(g_sum, g_all) < 2e-6
    eng.train_step(x[lo:hi], tr.enc_B, gt[lo:hi], spec, count=25000)
    assert torch.equal(eng.grads, g_all)  # (iii)
    out_a = tr.predict_all(chunk=1 << 18)
    out_b = tr.predict_all(chunk=100_003)
    assert out_a.shape == (3532800, 2) and torch.equal(out_a, out_b)  # (ii): rows are independent of their tile
    ref = reconstruct(tr.image, shape, False)
    assert ref.shape == (640, 368) and float(psnr(ref, ref)) > 80  # (iv): the reference psnr carries an eps in the MSE
    assert np.isfinite(tr.evaluate())


def test_full_size_trajectory_vs_oracle(dev):
    """BASELINE config 2 for real: SIREN 5x256 / gauss-512, 25 000-coordinate batches of the synthetic 640x368x15 k-space,
    six Adam steps through INRTrainer against the oracle's restatement of the train.py loop on the same rows (the
    oracle only ever sees the first 150 000 rows, which is all six sequential batches touch)."""
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    image, coords, shape = make_kspace(15, 640, 368, seed=1234, normalization="coil")
    cfg = dict(model="SIREN", loss="L2", lr=3e-5, batch_size=25000, max_epoch=1000, weight_decay=0.0, beta1=0.9,
               beta2=0.999, net=FULL_NET, encoder=FULL_ENC)
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=0)
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    n = 6 * 25000
    want = O.train_single_scale(cfg, sd, tr.encoder.B.cpu(), coords[:n], image[:n], 6)
    got = np.array([s[1] for s in tr.fit(6, log_every=1)])
    np.testing.assert_allclose(got, np.array(want), rtol=1e-5)
    flat = torch.cat([sd[k].reshape(-1) for k in tr.model.state_dict().keys()])
    assert rel_l2(tr.engine.params.cpu(), flat) < 1e-5
