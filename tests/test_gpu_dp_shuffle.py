"""Shuffled epochs under data parallelism -- ``-m gpu``, the pattern of test_gpu_dp.py: two processes share cuda:0 and
exchange through gloo.  Every rank fills its own epoch buffers from (shuffle_seed, epoch) with no communication and takes
its contiguous shard of each shuffled batch; two ranks must equal one rank with the same shuffle up to summation order,
at the tolerances test_gpu_dp.py holds its ragged-batch case ('siren', 333-row batches of 960 rows) to."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

NET = dict(network_input_size=32, network_output_size=2, network_depth=3, network_width=32, last_tanh=True)
ENC = dict(embedding="gauss", scale=2, embedding_size=16, coordinates_size=3)
BASE = dict(loss="L2", lr=1e-3, max_epoch=2, weight_decay=0.0, beta1=0.9, beta2=0.999, net=NET, encoder=ENC,
            shuffle=True, shuffle_seed=31)
SHAPE = (2, 24, 20)
CASES = {
    "siren": dict(BASE, model="SIREN", batch_size=333),
    "siren_hdr_masked": dict(BASE, model="SIREN", loss="HDR", batch_size=333),
    "fourier": dict(BASE, model="Fourier", batch_size=400),
    "multiscale": dict(BASE, model="MultiscaleKFourier", batch_size=400, partition=dict(no_steps=20, no_models=4),
                       net=dict(NET, network_depth=8)),
    "tv": dict(BASE, model="SIREN", batch_size=1, per_coil=True, use_tv=True, undersampling="grid-2*2"),
}


def _run(case, rank, world, pg=None):
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    from inr_mi355x.train_kspace_multiscale import MultiscaleTrainer
    cfg = CASES[case]
    image, coords, shape = make_kspace(*SHAPE)
    dev = torch.device("cuda:0")
    if case == "multiscale":
        dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
        tr = MultiscaleTrainer(cfg, image, coords, dist, None, shape, dev, seed=1, rank=rank, world=world, process_group=pg)
    else:
        mask = None
        if case.endswith("_masked"):
            mask = torch.rand(coords.shape[0], generator=torch.Generator().manual_seed(6)) < 0.6
        tr = INRTrainer(cfg, image, coords, shape, dev, seed=1, rank=rank, world=world, process_group=pg, mask=mask)
    assert tr.shuffle and tr.shuffle_seed == 31
    losses = [s[1] for s in tr.fit(5, log_every=1)]  # crosses into the second epoch: a second order, a second refill
    return losses, tr.engine.params.detach().cpu().clone()


def _worker(rank, world, port, case, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _run(case, rank, world)
        q.put((rank, res[0], res[1].numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_ranks_equal_one_with_shuffle(case):
    assert torch.cuda.is_available()
    world = 2
    ref_losses, ref_params = _run(case, 0, 1)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        rank, losses, params = q.get(timeout=300)
        got[rank] = (losses, params)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in range(world):
        losses, params = got[rank]
        np.testing.assert_allclose(np.array(losses), np.array(ref_losses), rtol=2e-5, err_msg=f"{case} rank {rank}")
        np.testing.assert_allclose(params, ref_params.numpy(), rtol=2e-4, atol=2e-6, err_msg=f"{case} rank {rank}")
    np.testing.assert_array_equal(got[0][1], got[1][1])  # replicas stay bitwise identical
