"""Every wrapper module whose library calls go through ``_lib.launch`` (``-m gpu``): the smallest valid call of one of
its entries, issued inside ``torch.cuda.stream(s)`` on a stream of its own.  ``launch`` hands torch's current stream to
the library as the entry's last argument.

Stream ``s`` is kept busy ahead of the call (torch.cuda._sleep: a spin kernel of a fixed number of clock ticks, far
longer than a wrapper takes on the host; the inputs are made before it, so nothing in the call waits on a copy).  Then:
  * the call returns while ``s`` is still busy (``not s.query()``): it was enqueued, it did not synchronise -- except
    sampling.row_cdf, which reads its totals back and so has waited for ``s`` by design;
  * after ``s.synchronize()`` the result has the bits of the same call on the default stream;
  * for one entry that takes its output buffer (gain_apply), the buffer still holds what was put there when it is
    read on the default stream BEFORE ``s.synchronize()``: the kernel sits on ``s`` behind the spin, not on the null
    stream, where it would have run at once.  torch's side streams do not wait for the null stream, nor it for them.
The sleep only has to outlast a host call; no bound on any duration is asserted.

Shapes: B = 3 rows (odd: the half-pair tail of the gain and mix kernels) or 2 x 3 x 5 pixels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, G, H, W = 3, 2, 3, 5
SPIN = 40_000_000  # clock ticks the side stream spins ahead of the call: tens of milliseconds at the least


def _t(*shape, seed=0, dtype=torch.float32):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5).to(dtype)


# per module: (inputs(dev) -> tuple of device tensors, call(*inputs) -> tuple of device tensors)
def _gain_in(dev):
    return _t(B, 2).to(dev), _t(B, seed=1).to(dev), _t(B, 2, seed=2).to(dev)


def _gain(y, s, gt):
    from inr_mi355x.engine import LossSpec
    from inr_mi355x.gain import gain_apply, gain_loss_grad
    return gain_loss_grad(LossSpec(), y, s, gt, B) + (gain_apply(y, s),)


def _mix_in(dev):
    return (_t(B, 2).to(dev), _t(B, 2, seed=1).to(dev), _t(B, 2, seed=3).to(dev), _t(B, 2, seed=4).to(dev),
            torch.tensor([0.1, 0.6, 0.9], device=dev))


def _mix(y0, y1, w, gt, dist):
    from inr_mi355x.engine import LossSpec
    from inr_mi355x.mix import mix_apply, mix_loss_grad
    out, res, dys, dw = mix_loss_grad(LossSpec(), [y0, y1], w, gt, dist, [0.0, 0.5, 1.5], [1 / 3, 1.0, 0.5])
    return out[:4], res, dys[0], dys[1], dw, mix_apply([y0, y1], w)


def _sense_in(dev):
    return _t(H * W, 2).to(dev), _t(G * H * W, 2, seed=1).to(dev), _t(G, H, W, 2, seed=2).to(dev)


def _sense(img, sens, gx):
    from inr_mi355x.sense import sense_apply, sense_grad
    return (sense_apply(img, sens, G, H, W, 1.5, 1),) + sense_grad(img, sens, gx, G, H, W, 1.5, 1)


def _sense_calib(img, sens, gx):
    from inr_mi355x.sense_calib import sense_adjoint
    return (sense_adjoint(sens, gx, G, H, W, 1.5, 1),)


def _sense_prior(img, sens, gx):
    from inr_mi355x.sense_prior import image_tv
    dimg = torch.zeros(H * W, 2, device=img.device)
    return image_tv(img, H, W, 0.1, 1e-3, dimg=dimg), dimg


def _focal(y, s, gt):
    from inr_mi355x.focal import FocalSpec, focal_loss_grad
    return focal_loss_grad(FocalSpec(), y, gt, B)


def _grid_in(dev):
    return (torch.empty(0, device=dev),)


def _grid(where):
    from inr_mi355x.grid import GridSpec, grid_rows
    return grid_rows(GridSpec(G, H, W), 0, G * H * W, device=where.device)


def _trajectory_in(dev):
    return _t(G, H, W, 2).to(dev), _t(B, 2, seed=1, dtype=torch.float64).to(dev)


def _trajectory(img, pos):
    from inr_mi355x.trajectory import nudft
    return (nudft(img, pos),)


def _coils(img, pos):
    from inr_mi355x.coils import coil_gram_device
    return (coil_gram_device(img, (G, H, W)).clone(),)


def _rows_in(dev):
    return torch.tensor([0.1, 0.6, 0.9], device=dev), _t(B, 2).to(dev), _t(B, 2, seed=1).to(dev)


def _ringnorm(dist, a, b):
    from inr_mi355x.ringnorm import ring_scale
    return (ring_scale(dist, a, [0.0, 0.5, 1.5], [2.0, 4.0]),)


def _bands(dist, a, b):
    from inr_mi355x.bands import band_stats_device
    return (band_stats_device(dist, a, b, None, 1, [(0.0, 0.5), (0.5, 1.5)])[2].clone(),)


def _sampling(dist, a, b):
    from inr_mi355x.sampling import row_cdf
    return (row_cdf(dist, scale=1024.0).cdf,)


CASES = {"gain": (_gain_in, _gain), "mix": (_mix_in, _mix), "sense": (_sense_in, _sense),
         "sense_calib": (_sense_in, _sense_calib), "sense_prior": (_sense_in, _sense_prior), "focal": (_gain_in, _focal),
         "grid": (_grid_in, _grid), "trajectory": (_trajectory_in, _trajectory), "coils": (_trajectory_in, _coils),
         "ringnorm": (_rows_in, _ringnorm), "bands": (_rows_in, _bands), "sampling": (_rows_in, _sampling)}
READS_BACK = ("sampling",)  # row_cdf returns host numbers: it has synchronised with its stream when it returns


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _same_bits(g, w):
    return g.shape == w.shape and g.dtype == w.dtype and \
        torch.equal(g.view(torch.uint8) if g.dim() else g, w.view(torch.uint8) if w.dim() else w)


@pytest.mark.parametrize("module", sorted(CASES))
def test_call_is_enqueued_on_the_current_stream(dev, module):
    make, call = CASES[module]
    inputs = make(dev)
    want = call(*inputs)  # default stream; also the first launches and allocations
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        torch.cuda._sleep(SPIN)
        got = call(*inputs)
        busy = not s.query()
    s.synchronize()
    assert busy or module in READS_BACK, "the call waited for its stream"
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), (module, i)


def test_the_kernel_waits_on_the_side_stream_not_on_the_null_stream(dev):
    from inr_mi355x.gain import gain_apply
    y, s_in, _ = _gain_in(dev)
    want = gain_apply(y, s_in)
    out = torch.full_like(y, 123.0)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        torch.cuda._sleep(SPIN)
        gain_apply(y, s_in, out=out)
    early = out.cpu()  # read on the default stream while ``s`` still spins
    busy = not s.query()
    s.synchronize()
    assert busy, "the side stream had run dry before the early read: nothing was shown"
    assert bool((early == 123.0).all()), "the kernel ran before its stream reached it"
    assert _same_bits(out, want)
