"""Shapes, seeded inputs and recorded figures shared by tests/test_sense_calib_host.py and tests/test_gpu_sense_calib.py
(DESIGN.md 4.29)."""
import numpy as np

from aux_bits_cases import rnd

# (C, H, W) x (a, b): W/2 odd (single-pixel path); the pair path with an odd block; odd H and W; the widest block over
# more than one column tile of 64 (three tiles, the last one partial); C = 1 and C = 5 (remainders of the coil loop's
# unroll by four)
KERNEL_CASES = (((3, 12, 10), (4, 4)), ((3, 8, 16), (5, 3)), ((2, 9, 7), (2, 2)), ((4, 6, 132), (4, 64)),
                ((1, 8, 12), (3, 4)), ((5, 70, 8), (6, 2)))
CASE_IDS = ["x".join(map(str, s)) + "_" + "x".join(map(str, k)) for s, k in KERNEL_CASES]
SCALE = 0.37
AMP = 0.3
FLOORS = (0.0, 0.8)  # the second removes pixels in every case above (12 of 120 ... 57 of 63 are kept)

# the trainer's set-up
FIT_SHAPE = (3, 12, 10)
FIT_BLOCK = [4, 4]
CG_ITERS = 3

# CG-SENSE, 3 iterations on the trainer's set-up (synthetic.make_kspace(3, 12, 10), grid-3*2 plus the 4 x 4 block, maps
# from the hann-windowed block): the relative L2 distance of the last iterate of the fp32 numpy operators
# (cg_sense_numpy(fp32=True): sense_apply_numpy, numpy's complex64 FFT, sense_adjoint_numpy) from the float64 iterations,
# measured on the host by tests/test_sense_calib_host.py::test_cg_fp32_operators_distance_is_the_recorded_one.  The GPU
# test allows 8 x this and never less than 1e-5: rocFFT and pocketfft round differently and CG amplifies the difference.
CG_FP32_REL_L2 = 5.9e-7  # measured: 5.82e-7 (after iterations 1, 2, 3: 7.0e-8, 2.8e-7, 5.8e-7)
CG_FLOOR_TOL = 1e-5


def kspace(C, H, W, seed=0, amp=AMP):
    """fp32 [C,H,W,2]: a seeded centred k-space"""
    return rnd(C * H * W * 2, 71 + seed, amp).reshape(C, H, W, 2)


def adjoint_inputs(G, H, W, seed=0, amp=AMP):
    """sens [G*H*W,2], gx [G,H,W,2], img [H*W,2] fp32 (img: for inr_sense_grad on the same inputs)"""
    n = H * W
    return (rnd(G * n * 2, 72 + seed, amp).reshape(G * n, 2), rnd(G * n * 2, 73 + seed, amp).reshape(G, H, W, 2),
            rnd(n * 2, 74 + seed, amp).reshape(n, 2))


def grid_mask(H, W, gx=3, gy=2):
    """bool [H,W]: undersampling.grid_mask as numpy"""
    from inr_mi355x.undersampling import grid_mask as gm
    return gm(H, W, gx, gy).numpy() != 0


def fit_problem():
    """(maps complex128 [C,H,W], y complex128 [C,H,W], mask bool [C,H,W], block fp32 [C,a,b,2]) of the trainer's set-up,
    from the host alone; the maps are the fp32 text of the kernels (what the device holds, bit for bit), widened"""
    from inr_mi355x import sense_calib as K
    from inr_mi355x.synthetic import make_kspace
    C, H, W = FIT_SHAPE
    k = make_kspace(C, H, W)[0].reshape(C, H, W, 2).numpy()
    mask = np.broadcast_to(K.add_acs(grid_mask(H, W), *FIT_BLOCK)[None], (C, H, W))
    block = K.cut_block(k, *FIT_BLOCK, "hann")
    m32, _ = K.calibrate_numpy(block, H, W, fp32=True)
    maps = (m32[..., 0].astype(np.float64) + 1j * m32[..., 1]).reshape(C, H, W)
    return maps, k[..., 0].astype(np.float64) + 1j * k[..., 1], mask, block

