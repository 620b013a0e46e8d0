"""Shared inputs of test_nufft_host.py and test_gpu_nufft.py (Kaiser-Bessel gridding): shapes, sample
counts, positions, samples and weights, all from fixed seeds."""
import numpy as np

SHAPES = [(1, 6, 5), (3, 7, 8), (2, 40, 36), (1, 70, 66)]  # the last: 140 x 132 cells, 9 x 9 spread tiles, partial edges
HOST_SHAPES = SHAPES[:3]
COUNTS = [1, 63, 65, 257]  # around the 64-sample LDS chunk and the 64-sample padding of the taps


def positions(H, W, M, seed):
    """integers, half-integers, the corners 0 and n - 1 (whose taps wrap), values outside the grid and arbitrary
    fractions"""
    g = np.random.default_rng(seed)
    fixed = [(0.0, 0.0), (H - 1.0, W - 1.0), (0.0, W - 1.0), (H - 1.0, 0.0), (H // 2, W // 2), (0.5, W - 1.5),
             (H - 0.5, -0.5), (-3.0, W + 2.0), (2.0 * H + 1.25, -1.75 * W), (1.0, 2.0), (H / 2 - 0.5, 0.25)]
    pos = np.empty((M, 2), dtype=np.float64)
    for m in range(M):
        if m < len(fixed) and M > 1:
            pos[m] = fixed[m]
        elif m % 3 == 0:
            pos[m] = (g.integers(0, H), g.integers(0, W))
        elif m % 3 == 1:
            pos[m] = (g.integers(0, 2 * H) / 2.0, g.integers(0, 2 * W) / 2.0)
        else:
            pos[m] = (g.uniform(-H, 2 * H), g.uniform(-W, 2 * W))
    if M == 1:
        pos[0] = (H / 2 - 0.5, 0.25)
    return pos


def one_cell(H, W, M, seed):
    """M distinct positions whose floor(g) is one grid cell: one bin holds every sample, every other bin is empty"""
    g = np.random.default_rng(seed)
    pos = np.empty((M, 2), dtype=np.float64)
    pos[:, 0] = H // 2 + 0.5 * g.uniform(0.0, 1.0, M) * (1.0 - 2.0 ** -20)  # g_y in [H, H + 1)
    pos[:, 1] = W // 2 + 0.5 * g.uniform(0.0, 1.0, M) * (1.0 - 2.0 ** -20)
    return pos


def images(C, H, W):
    g = np.random.default_rng(C * 100 + H)
    return (g.standard_normal((C, H, W)) + 1j * g.standard_normal((C, H, W))).astype(np.complex64)


def samples(C, M):
    g = np.random.default_rng(C * 1000 + M)
    normal = (g.standard_normal((C, M)) + 1j * g.standard_normal((C, M))).astype(np.complex64)
    single = np.zeros((C, M), dtype=np.complex64)
    for c in range(C):
        single[c, (M // 2 + c) % M] = 0.75 - 1.25j  # one non-zero sample, another one per coil
    return {"normal": normal, "single": single}


def weights(M):
    return np.random.default_rng(M).uniform(0.25, 4.0, M).astype(np.float32)
