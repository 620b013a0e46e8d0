"""The LDS options inr_mlp_kernel's launcher takes from csrc/inr_lds.h (``-m gpu``).  For the 256-wide instantiation
(NB = 8, four waves: 147 456 B of images) the last-layer fragments (MlpArgs::ll_lds, 4 112 B) and the fused step's dZ_last
images (MlpArgs::dz_lds, 4 608 B) sit behind the [E][3] encoder matrix only while they fit the CU's 160 KiB: the dZ_last
images up to enc_size 632, the fragments up to 1016 (tools/probes/lds_layout_check.cpp prints the first sizes without them,
640 and 1024; tests/test_lds_layout_host.py pins them).  One forward and one fused step on either side of both thresholds,
against the float64 evaluation and under the tolerances tests/test_gpu_parity.py holds SIREN behind the gauss encoder to;
INR_RS=0 keeps the step in inr_mlp_kernel at enc_size 256 too, where the plan also has the row-split kernel."""
import ctypes as C

import pytest
import torch

import test_gpu_parity as P

pytestmark = pytest.mark.gpu

NET = dict(network_output_size=2, network_depth=3, network_width=256, last_tanh=True)  # 3 Linear layers
ROWS = 3 * 128 + 17  # three full tiles and a ragged one
DZ_OFF, LL_OFF, BASE_OFF = 640, 1024, 1368  # first enc_size without dz_lds / without ll_lds / the launcher refuses


def _setup(E, dev):
    import inr_mi355x as M
    net = dict(NET, network_input_size=2 * E)
    torch.manual_seed(E)
    enc = M.Positional_Encoder(dict(embedding="gauss", scale=2, embedding_size=E, coordinates_size=3), device=dev)
    model = M.SIREN(net)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    coords = torch.rand(ROWS, 3, generator=g) * 2 - 1
    gt = torch.randn(ROWS, 2, generator=g) * 0.2
    return net, enc, model.to(dev), sd, coords, gt


@pytest.mark.parametrize("E", [256, DZ_OFF, LL_OFF])
def test_forward_and_step_on_both_sides_of_the_option_thresholds(E, monkeypatch):
    import inr_mi355x as M
    from inr_mi355x import _lib as L
    dev = torch.device("cuda:0")
    monkeypatch.setenv("INR_RS", "0")
    net, enc, model, sd, coords, gt = _setup(E, dev)
    ref_out, ref_loss, ref_grad = P._oracle_grads({k: v.double() for k, v in sd.items()}, enc.B.cpu().double(),
                                                  coords.double(), gt.double(), net)
    eng = model.fused_engine(E)
    info = L.StepInfo()
    L.check(eng.lib.inr_plan_step_info(eng.plan, ROWS, C.byref(info)))
    assert info.row_split == 0 and info.hidden_blocks == 8
    out = eng.forward(coords.to(dev), enc.B.contiguous(), save=False).cpu()
    loss = eng.train_step(coords.to(dev), enc.B.contiguous(), gt.to(dev), M.LossSpec(L.LOSS_L2_HALF)).cpu()
    got = eng.grads.cpu()
    print(f"E {E}: out rel-L2 {P.rel_l2(out, ref_out):.3e} max abs {float((out.double() - ref_out).abs().max()):.3e}, "
          f"loss rel {abs(float(loss) - float(ref_loss)) / float(ref_loss):.3e}, grad rel-L2 {P.rel_l2(got, ref_grad):.3e} "
          f"max abs {float((got.double() - ref_grad).abs().max()):.3e} of {float(ref_grad.abs().max()):.3e}")
    # tests/test_gpu_parity.py, test_full_size_siren_vs_oracle
    torch.testing.assert_close(out, ref_out.float(), rtol=1e-5, atol=2e-6)
    assert P.rel_l2(out, ref_out) < 1e-5
    torch.testing.assert_close(loss.reshape(()), ref_loss.float(), rtol=1e-5, atol=0)
    assert P.rel_l2(got, ref_grad) < 1e-5
    torch.testing.assert_close(got, ref_grad.float(), rtol=1e-3, atol=float(ref_grad.abs().max()) * 1e-5)


def test_a_refused_launch_leaves_the_next_call_working():
    """enc_size 1368: images + encoder matrix alone exceed the CU's LDS.  The launcher refuses on the host, the call returns
    the library's error, and a valid plan's forward afterwards is as good as ever."""
    dev = torch.device("cuda:0")
    _, enc, model, _, coords, _ = _setup(BASE_OFF, dev)
    eng = model.fused_engine(BASE_OFF)
    with pytest.raises(RuntimeError, match="libinr_mi355x: error"):
        eng.forward(coords.to(dev), enc.B.contiguous(), save=False)
    net, enc, model, sd, coords, gt = _setup(256, dev)
    ref_out, _, _ = P._oracle_grads({k: v.double() for k, v in sd.items()}, enc.B.cpu().double(), coords.double(),
                                    gt.double(), net)
    out = model.fused_engine(256).forward(coords.to(dev), enc.B.contiguous(), save=False).cpu()
    torch.cuda.synchronize()
    torch.testing.assert_close(out, ref_out.float(), rtol=1e-5, atol=2e-6)
