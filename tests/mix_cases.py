"""Shared inputs of tests/test_mix_host.py and tests/test_gpu_mix.py (mixture of heads): pure numpy, made
from exact integer hashes (aux_bits_cases.rnd), so both files and every run see the same bits.

Sizes: the edges of the kernel's partition of row pairs over its blocks (1, 63, 64, 255, 256, 257) and one row past 64 x
256.  Heads: 2, 3 (odd: the 8-byte accesses to w), 4, 8 (the largest).  w is uniform in (-0.5, 1.5): the sigmoid only gives
(0, 1) and the kernel must not rely on that.  y has amplitude 0.3 in one set (the clamp is idle at K <= 4) and 1.0 in the
other (the clamp acts on many rows).  The radii are K equal rings up to 1.2; dist is uniform up to 1.26 (some rows lie
beyond the last ring: they are in the mixed term alone), with every 37th row exactly ON a ring edge (it counts in both
rings); at B = 63 ring 1 is empty (its rows are moved into ring 0, the edge rows onto radii[0]); at B = 1 the row sits on
radii[1].

The msle kind takes log(y + 1 + 1e-9): its y and gt are made positive (as tests/test_gpu_gain.py does) and so is its w,
since a negative weight could take pre to -1 and below, where the loss is not defined in any precision.
"""
import numpy as np

from aux_bits_cases import rnd

SIZES = (1, 63, 64, 255, 256, 257, 16385)
HEADS = (2, 3, 4, 8)
MASKS = ("none", "random", "ones", "zeros")
AMPS = (0.3, 1.0)
EDGE_EVERY = 37
NEAR_CLAMP = 1e-6  # rows whose float64 |pre_c| is this close to 1 may fall on either side of the clamp in fp32
NEAR_CAP = 0.01    # ... and must be at most this share of the rows


def radii_of(K):
    return [float(np.float32(1.2 * k / K)) for k in range(K + 1)]


def rows(kind, B, K, amp):
    """(ys K x [B,2], w [B,K], gt [B,2], dist [B], radii) as fp32"""
    ys = [rnd(B * 2, 101 + k, amp).reshape(B, 2) for k in range(K)]
    gt = rnd(B * 2, 120, amp).reshape(B, 2)
    w = rnd(B * K, 121, 1.0).reshape(B, K) + np.float32(0.5)
    if kind == "msle":
        ys = [np.abs(y) + np.float32(0.05) for y in ys]
        gt, w = np.abs(gt) + np.float32(0.05), np.abs(w)
    radii = radii_of(K)
    r32 = np.asarray(radii, dtype=np.float32)
    dist = (np.abs(rnd(B, 122, 1.26))).astype(np.float32)
    edge = np.arange(B) % EDGE_EVERY == 0
    dist[edge] = r32[(np.arange(B)[edge] // EDGE_EVERY) % (K + 1)]
    if B == 1:
        dist[0] = r32[1]
    if B == 63:  # ring 1 empty
        dist[edge] = r32[0]
        inside = (dist >= r32[1]) & (dist <= r32[2])
        dist[inside] = np.float32(0.5) * (r32[0] + r32[1])
    return ys, w.astype(np.float32), gt, dist, radii


def mask_of(tag, B):
    if tag == "none":
        return None
    if tag == "random":
        m = (rnd(B, 123) > 0).astype(np.uint8)
        m[0] = 1
        return m
    return (np.ones if tag == "ones" else np.zeros)(B, dtype=np.uint8)


def near_clamp(pre64):
    """bool [B]: a component of the float64 pre lies within NEAR_CLAMP of +-1"""
    return (np.abs(np.abs(pre64) - 1.0) <= NEAR_CLAMP).any(axis=1)
