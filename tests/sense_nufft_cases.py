"""Shapes, seeded inputs and recorded figures shared by tests/test_sense_nufft_host.py and tests/test_gpu_sense_nufft.py
(off-grid SENSE fits on calibrated maps)."""
import numpy as np

from aux_bits_cases import rnd

# (G, H, W): W/2 odd (single-cell path); the pair path; odd H and W (H - H//2 centring differs from H/2); G = 1 and
# G = 5 (remainders of the coil loop's unroll by four); H at the gridding minimum with more than one block per row
KERNEL_SHAPES = ((3, 12, 10), (3, 8, 16), (2, 9, 7), (1, 8, 12), (5, 6, 8), (4, 3, 132))
SHAPE_IDS = ["x".join(map(str, s)) for s in KERNEL_SHAPES]
M = 37
SCALE = 0.37
AMP = 0.3

# the trainer's set-up
FIT_SHAPE = (3, 12, 10)
FIT_BLOCK = [4, 4]
FIT_TRAJECTORY = "spokes-16"
CG_ITERS = 3

# Off-grid calibration on the host, synthetic.make_kspace(3, 24, 20) sampled on spokes-40 (exact NUDFT), ramp density:
# nudft_adjoint_numpy -> fft2c -> cut_block(CALIB_BLOCK, hann) -> calibrate_numpy, against the maps
# calibrated on the Cartesian centre of the same scan.  The relative L2 distance of the two map sets, measured by
# tests/test_sense_nufft_host.py::test_offgrid_calibration_distance_is_the_recorded_one.  A property of the trajectory,
# not a pass mark: the test asserts that the figure is reproduced.
CALIB_SHAPE = (3, 24, 20)
CALIB_TRAJECTORY = "spokes-40"
CALIB_BLOCK = [8, 8]
CALIB_REL_L2 = 0.466  # measured: 4.6597e-01 (40 spokes over 24 x 20: the ramp-weighted adjoint is far from the centre)

# Non-Cartesian CG-SENSE, 3 iterations on the trainer's set-up: the relative L2 distance of the last iterate of
# cg_sense_nufft_numpy(fp32=True) from the float64 iterations, measured on the host by
# tests/test_sense_nufft_host.py::test_cg_fp32_operators_distance_is_the_recorded_one.  The GPU test allows 8 x this and
# never less than 1e-5, as tests/test_gpu_sense_calib.py does for the Cartesian baseline.
CG_FP32_REL_L2 = 3.0e-7  # measured: 2.997e-7 (after iterations 1, 2, 3: 1.3e-7, 1.7e-7, 3.0e-7)
CG_FLOOR_TOL = 1e-5


def positions(H, W, seed=0):
    """fp64 [M, 2]: exact integers, a position within one cell of each grid edge (taps that wrap on the oversampled
    grid), two samples in one cell, and seeded fractions inside the grid"""
    g = np.random.default_rng(1000 * H + W + seed)
    fixed = [(0.0, 0.0), (H - 1.0, W - 1.0), (H // 2, W // 2), (1.0, 2.0),  # integers
             (0.25, W / 2.0), (H - 1.25, W / 2.0), (H / 2.0, 0.3), (H / 2.0, W - 1.2),  # near each edge
             (H / 2.0 + 0.10, W / 2.0 + 0.10), (H / 2.0 + 0.15, W / 2.0 + 0.20)]  # one cell: g = 2 u + const
    pos = np.empty((M, 2), dtype=np.float64)
    pos[:len(fixed)] = fixed
    pos[len(fixed):, 0] = g.uniform(0.0, H - 1.0, M - len(fixed))
    pos[len(fixed):, 1] = g.uniform(0.0, W - 1.0, M - len(fixed))
    return pos


def operands(G, H, W, seed=0):
    """img [H*W,2], maps [G*H*W,2], grid [G,2H,2W,2] (a seeded one for finish and interp), val [G,M,2], weights [M]:
    fp32"""
    n = H * W
    return (rnd(n * 2, 91 + seed, AMP).reshape(n, 2), rnd(G * n * 2, 92 + seed, AMP).reshape(G * n, 2),
            rnd(G * n * 8, 93 + seed, AMP).reshape(G, 2 * H, 2 * W, 2), rnd(G * M * 2, 94 + seed, AMP).reshape(G, M, 2),
            (np.abs(rnd(M, 95 + seed, 1.0)) + np.float32(0.25)).astype(np.float32))


def fit_samples():
    """(maps complex128 [C,H,W], y complex128 [C,M], pos [M,2], weights [M], block fp32 [C,a,b,2]) of the trainer's
    set-up from the host alone: the exact NUDFT samples of synthetic.make_kspace's coil images on FIT_TRAJECTORY, the
    block cut from their density-weighted exact adjoint, the maps the fp32 text of the calibration kernels, widened"""
    from inr_mi355x import sense_calib as K
    from inr_mi355x import trajectory as T
    from inr_mi355x.sense import fft2c_numpy
    from inr_mi355x.synthetic import make_kspace
    C, H, W = FIT_SHAPE
    k = make_kspace(C, H, W)[0].reshape(C, H, W, 2).numpy()
    parsed = T.parse_trajectory(FIT_TRAJECTORY)
    pos = T.positions(parsed, H, W)
    w = T.parse_density(None, parsed, H, W)[1]
    img = fft2c_numpy(k[..., 0].astype(np.float64) + 1j * k[..., 1], inverse=True)
    y = T.nudft_numpy(img, pos)
    back = fft2c_numpy(T.nudft_adjoint_numpy(y, pos, H, W, w))
    block = K.cut_block(np.stack((back.real, back.imag), -1), *FIT_BLOCK, "hann")
    m32, _ = K.calibrate_numpy(block, H, W, fp32=True)
    maps = (m32[..., 0].astype(np.float64) + 1j * m32[..., 1]).reshape(C, H, W)
    return maps, y, pos, w, block
