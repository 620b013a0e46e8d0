"""Shapes and seeded inputs shared by tests/test_sense_prior_host.py and tests/test_gpu_sense_prior.py."""
import numpy as np

from aux_bits_cases import rnd

AMP = 0.3
WEIGHT = 0.37
# (H, W): W even with W/2 odd and even (the pair path), odd H and W (one pixel per lane), a wide and a tall image, W = 66;
# then the degenerate axes
SHAPES = ((12, 10), (9, 7), (6, 132), (70, 8), (5, 66), (1, 8), (8, 1), (2, 2))
# odd W: one pixel per lane, H * W = 65535 units > IMAGE_TV_BLOCKS * IMAGE_TV_THREADS = 255 * 256 = 65280 lanes -- the
# launch is capped at 255 blocks and the first 255 lanes take a second grid-stride turn
LARGE = (257, 255)
EPS = (1e-3, 0.1, 0.0)
CASES = tuple((s, e) for s in SHAPES + (LARGE,) for e in EPS)
CASE_IDS = [f"{h}x{w}_eps{e:g}" for (h, w), e in CASES]
PATCH = 3  # eps = 0: a constant PATCH x PATCH block (clipped to the image) makes n = 0 on its upper-left pixels

# the trainer's set-up: sense_calib_cases.FIT_SHAPE (3, 12, 10), block 4 x 4, grid-3*2
FIT_EPS = 1e-3


def image(H, W, eps, seed=0, amp=AMP):
    """fp32 [H*W,2]: a seeded complex image; with eps == 0 a constant block is pasted in at (1, 1) (at (0, 0) where an axis
    is shorter than PATCH + 1), so that n = 0 occurs"""
    img = rnd(H * W * 2, 91 + seed, amp).reshape(H, W, 2).copy()
    if eps == 0:
        y0, x0 = (1 if H > PATCH else 0), (1 if W > PATCH else 0)
        img[y0:y0 + PATCH, x0:x0 + PATCH] = np.float32([0.125, -0.25])
    return img.reshape(H * W, 2)


def zero_n(H, W):
    """bool [H,W]: the pixels of image(H, W, 0) with n = 0 -- both forward differences vanish: the right (lower) neighbour
    is missing, or it and the pixel lie in the constant block.  The last pixel of the last row is always one."""
    y0, x0 = (1 if H > PATCH else 0), (1 if W > PATCH else 0)
    inside = np.zeros((H, W), dtype=bool)
    inside[y0:y0 + PATCH, x0:x0 + PATCH] = True
    right = np.ones((H, W), dtype=bool)
    right[:, :-1] = inside[:, :-1] & inside[:, 1:]
    down = np.ones((H, W), dtype=bool)
    down[:-1, :] = inside[:-1, :] & inside[1:, :]
    return right & down


def zero_grad(H, W):
    """bool [H,W]: where the rule gives a gradient of exactly 0 -- n = 0 at the pixel, and at its left and its upper
    neighbour where it has them"""
    z = zero_n(H, W)
    left = np.ones((H, W), dtype=bool)
    left[:, 1:] = z[:, :-1]
    up = np.ones((H, W), dtype=bool)
    up[1:, :] = z[:-1, :]
    return z & left & up


def dimg0(H, W, seed=0):
    """fp32 [H*W,2]: what dimg holds before an accumulating call"""
    return rnd(H * W * 2, 97 + seed, 0.01).reshape(H * W, 2)


def tv_torch(I, weight, eps):
    """weight * TV of a complex torch tensor I [H,W] (any real dtype behind it), written plainly with slicing and
    torch.sqrt: what autograd differentiates"""
    import torch
    H, W = I.shape
    ax2 = torch.zeros(H, W, dtype=I.real.dtype)
    ay2 = torch.zeros(H, W, dtype=I.real.dtype)
    if W > 1:
        dx = I[:, 1:] - I[:, :-1]
        ax2 = torch.nn.functional.pad(dx.real ** 2 + dx.imag ** 2, (0, 1))
    if H > 1:
        dy = I[1:, :] - I[:-1, :]
        ay2 = torch.nn.functional.pad(dy.real ** 2 + dy.imag ** 2, (0, 0, 0, 1))
    n = torch.sqrt(ax2 + ay2 + eps ** 2)
    return weight * (n - eps).sum() / (H * W)
