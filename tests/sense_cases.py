"""Shapes and seeded inputs shared by tests/test_sense_host.py and tests/test_gpu_sense.py."""
import numpy as np

from aux_bits_cases import rnd

PARITIES = (1, 2, 3, 4, 5, 8)  # shift_index against torch.fft.ifftshift for H, W in PARITIES x PARITIES
HOST_SHAPES = ((1, 1, 1), (2, 3, 5), (3, 4, 6))  # (G, H, W)
# (G, H, W) of the kernel tests: one pixel; one pair; both odd; W/2 odd (8-byte path); the 16-byte path; H odd on the
# 16-byte path; W/2 odd with G past the unroll; several blocks plus a partial one on the 16-byte path
KERNEL_SHAPES = ((1, 1, 1), (1, 2, 2), (3, 5, 7), (2, 6, 10), (4, 8, 12), (2, 7, 8), (8, 33, 66), (3, 129, 260))
SCALE = 0.37
AMP = 0.3  # the amplitude of tests/test_gpu_gain.py's rows
MASKS = ("none", "random", "zeros")


def inputs(G, H, W, seed=0, amp=AMP):
    """img [H*W,2], sens [G*H*W,2], gx [G,H,W,2] fp32"""
    n = H * W
    return (rnd(n * 2, 61 + seed, amp).reshape(n, 2), rnd(G * n * 2, 62 + seed, amp).reshape(G * n, 2),
            rnd(G * n * 2, 63 + seed, amp).reshape(G, H, W, 2))


def targets(kind, G, H, W, tag):
    """(gt [G*H*W,2], mask [G*H*W] uint8 or None, count) in the dataset's own order; msle: positive targets"""
    n = G * H * W
    gt = rnd(n * 2, 64, AMP).reshape(n, 2)
    if kind == "msle":
        gt = np.abs(gt) + np.float32(0.05)
    if tag == "none":
        return gt, None, n
    if tag == "zeros":
        return gt, np.zeros(n, dtype=np.uint8), 1  # nothing sampled, count = 1
    m = (rnd(n, 65) > 0).astype(np.uint8)
    m[0] = 1
    return gt, m, int(m.sum())
