"""Shuffled epochs, host side (no GPU): the keyed stateless permutation of DESIGN.md section 4.12 as restated in
inr_mi355x/shuffle.py, the per-coil coil order, and the settings a trainer refuses."""
import ctypes
import math

import numpy as np
import pytest
import torch

N_LIST = [1, 2, 3, 255, 256, 257, 25000, 15 * 640 * 368]


@pytest.mark.parametrize("n", N_LIST)
def test_epoch_order_is_a_bijection(n):
    from inr_mi355x.shuffle import epoch_order
    for seed, epoch in ((0, 0), (5, 3)):
        o = epoch_order(n, seed, epoch)
        assert o.dtype == np.int64 and o.shape == (n,)
        assert np.array_equal(np.sort(o), np.arange(n))


def test_epoch_order_differs_between_epochs_and_seeds():
    from inr_mi355x.shuffle import epoch_order
    for n in (255, 256, 257, 25000):
        a = epoch_order(n, 0, 0)
        for other in (epoch_order(n, 0, 1), epoch_order(n, 1, 0), epoch_order(n, 2 ** 32, 0), epoch_order(n, 0, 2)):
            assert np.mean(a == other) < 0.05, n  # a uniform pair of orders agrees at about 1 / n of the positions
        assert not np.array_equal(a, np.arange(n))


def test_epoch_order_is_stateless():
    """Equal (n, seed, epoch) give equal orders whatever was drawn before, from this module or any generator."""
    from inr_mi355x.shuffle import epoch_order
    want = epoch_order(25000, 7, 4)
    torch.manual_seed(123)
    np.random.seed(5)
    torch.randperm(1000)
    np.random.permutation(1000)
    for e in range(6):
        epoch_order(257, 7, e)
    assert np.array_equal(epoch_order(25000, 7, 4), want)
    assert np.array_equal(epoch_order(25000, 7 + 2 ** 64, 4 + 2 ** 32), want)  # seed modulo 2^64, epoch modulo 2^32


def test_epoch_order_pinned_values():
    """The text of section 4.12 pins the integers: a change of rounds, constants or key schedule shows up here."""
    from inr_mi355x.shuffle import domain_bits, epoch_order, round_keys
    assert [domain_bits(n) for n in (1, 256, 257, 1024, 1025, 15 * 640 * 368, 2 ** 31 - 1)] == [8, 8, 10, 10, 12, 22, 32]
    assert len(round_keys(0, 0)) == 6 and all(0 <= k < 2 ** 32 for k in round_keys(0, 0))
    assert epoch_order(3, 0, 0).tolist() == [1, 2, 0]
    assert epoch_order(257, 0, 0)[:8].tolist() == [130, 13, 164, 179, 85, 165, 1, 36]
    assert epoch_order(15 * 640 * 368, 0, 0)[:4].tolist() == [279994, 1907101, 2469925, 2617353]


def test_every_batch_sees_every_coil():
    """n = 15 * 640 * 368, bs = 25 000: every batch of epochs 0 and 1 holds rows of all 15 coils (a uniform order misses a
    coil in a batch with probability about 15 * (14/15)^25000); the sequential order fails the same check."""
    from inr_mi355x.shuffle import epoch_order
    C, hw, bs = 15, 640 * 368, 25000
    n = C * hw

    def coils_per_batch(order):
        coil = order // hw
        return [len(np.unique(coil[lo:lo + bs])) for lo in range(0, n, bs)]

    for epoch in (0, 1):
        per = coils_per_batch(epoch_order(n, 0, epoch))
        assert len(per) == math.ceil(n / bs) and min(per) == C, (epoch, min(per))
    assert max(coils_per_batch(np.arange(n))) <= 2


def test_coil_order_is_a_permutation():
    from inr_mi355x.shuffle import CoilOrder, coil_order
    for C in (1, 2, 15, 32):
        for epoch in range(4):
            assert sorted(coil_order(C, 3, epoch)) == list(range(C))
    assert len({tuple(coil_order(15, 3, e)) for e in range(8)}) == 8
    co = CoilOrder(15, 3)
    assert [co.at(2, it) for it in range(15)] == coil_order(15, 3, 2)
    assert [co.at(0, it) for it in range(15)] == coil_order(15, 3, 0)


def test_row_count_limit():
    from inr_mi355x.shuffle import epoch_order
    with pytest.raises(ValueError, match="2\\^31"):
        epoch_order(2 ** 31, 0, 0)
    with pytest.raises(ValueError):
        epoch_order(0, 0, 0)


def test_shuffle_settings_and_graph_steps_refusal():
    from inr_mi355x.shuffle import shuffle_settings
    from inr_mi355x.train import INRTrainer
    assert shuffle_settings({}, 4) == (False, 4)
    assert shuffle_settings({"shuffle": True}, 4) == (True, 4)
    assert shuffle_settings({"shuffle": True, "shuffle_seed": 9}, 4) == (True, 9)
    assert shuffle_settings({"shuffle": False}, 4, graph_steps=True) == (False, 4)
    image, coords = torch.zeros(8, 2), torch.zeros(8, 3)
    cfg = dict(model="SIREN", loss="L2", batch_size=4, shuffle=True)
    with pytest.raises(ValueError, match="graph_steps"):  # refused before anything touches a device
        INRTrainer(cfg, image, coords, (2, 2, 2), "cuda", graph_steps=True)


def test_cli_flags_set_the_config_keys():
    import argparse

    from inr_mi355x.train import add_shuffle_flags, apply_shuffle_flags
    ap = argparse.ArgumentParser()
    add_shuffle_flags(ap)
    assert apply_shuffle_flags({}, ap.parse_args([])) == {}
    assert apply_shuffle_flags({}, ap.parse_args(["--shuffle"])) == {"shuffle": True}
    assert apply_shuffle_flags({"shuffle": True}, ap.parse_args(["--shuffle-seed", "12"])) == {"shuffle": True,
                                                                                              "shuffle_seed": 12}


def test_abi_entry_refuses_bad_arguments_without_a_gpu():
    """inr_shuffle_epoch validates before it launches: these calls return an error and never reach the device."""
    from inr_mi355x import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    none = None

    def call(n, bs, coords=none, gt=none, coords_out=none, gt_out=none, counts=none, order=none):
        return lib.inr_shuffle_epoch(n, bs, 0, 0, coords, gt, none, none, coords_out, gt_out, none, none, counts, order, None)

    assert call(0, 1, order=fake) != 0
    assert "n = 0" in L.last_error()
    assert call(2 ** 31, 1, order=fake) != 0
    assert call(10, 1) != 0 and "no output" in L.last_error()
    assert call(10, 1, coords=fake) != 0 and "go together" in L.last_error()
    assert call(10, 1, coords=fake, coords_out=fake) != 0 and "in-place" in L.last_error()
    assert call(10, 0, counts=fake) != 0 and "batch_size" in L.last_error()
    assert call(10, 1, gt=ctypes.c_void_p(4100), gt_out=fake) != 0 and "aligned" in L.last_error()
