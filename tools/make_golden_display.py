#!/usr/bin/env python3
"""Generate tests/golden/display.npz by RUNNING the reference's own save_im and stats_per_coil (models/utils.py:254-287)
on small seeded inputs (build container only: needs the reference checkout, matplotlib, PIL and tabulate).

    python tools/make_golden_display.py /path/to/reference/src      (or INR_REFERENCE_SRC=/path/to/reference/src)

What is written is data only: the inputs, the R channel of every PNG save_im wrote (decoded with PIL), the float32 array
save_im handed to plt.imsave, matplotlib's own normalisation of it, the 256 bytes of matplotlib's 'gray' table, and the
numbers stats_per_coil put into its table.  models/utils.py imports h5py, skimage.metrics, torchvision and fastmri at
module scope; none of them is touched by the two functions, so empty stand-ins are registered, and fastmri.complex_abs /
fastmri.rss are their in-memory formulas, as tools/make_golden.py does it.
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
sys.dont_write_bytecode = True  # the reference tree is read-only: importing it must not leave __pycache__ behind


def import_reference_utils(ref_src):
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, ref_src)
    fm = types.ModuleType("fastmri")
    fm.complex_abs = lambda x: (x ** 2).sum(dim=-1).sqrt()
    fm.rss = lambda x, dim=0: torch.sqrt((x ** 2).sum(dim))
    fm.data = types.ModuleType("fastmri.data")
    fm.data.transforms = types.ModuleType("fastmri.data.transforms")
    sk = types.ModuleType("skimage")
    sk.metrics = types.ModuleType("skimage.metrics")
    sk.metrics.structural_similarity = None
    tv = types.ModuleType("torchvision")
    tv.utils = types.ModuleType("torchvision.utils")
    tv.transforms = types.ModuleType("torchvision.transforms")
    for name, mod in (("fastmri", fm), ("fastmri.data", fm.data), ("fastmri.data.transforms", fm.data.transforms),
                      ("skimage", sk), ("skimage.metrics", sk.metrics), ("torchvision", tv),
                      ("torchvision.utils", tv.utils), ("torchvision.transforms", tv.transforms),
                      ("h5py", types.ModuleType("h5py"))):
        sys.modules.setdefault(name, mod)
    import models.utils as mu
    return mu


def decode_r(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGBA"))[:, :, 0].copy()


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("INR_REFERENCE_SRC")
    if not ref_src:
        sys.exit("usage: make_golden_display.py REFERENCE_SRC")
    mu = import_reference_utils(ref_src)
    import matplotlib
    import matplotlib.colors
    import matplotlib.pyplot as plt
    torch.set_num_threads(1)

    handed = []  # what save_im hands to plt.imsave: (float array, vmin, vmax)
    real_imsave = plt.imsave

    def imsave(fname, arr, **kw):
        handed.append((np.array(arr, copy=True), kw.get("vmin"), kw.get("vmax")))
        return real_imsave(fname, arr, **kw)

    plt.imsave = imsave
    rows_seen = []
    real_tabulate = mu.tabulate

    def tabulate(rows, headers=()):
        rows_seen.append([tuple(float(v) for v in r) for r in rows])
        return real_tabulate(rows, headers=headers)

    mu.tabulate = tabulate

    g = torch.Generator().manual_seed(20)
    C, H, W = 4, 24, 20
    # magnitudes over several decades, a bright centre, as a real scan's k-space
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    envelope = torch.exp(-9.0 * torch.sqrt(yy ** 2 + xx ** 2))
    gains = torch.tensor([1.0, 0.3, 2.5, 0.05])[:, None, None, None]
    kspace = torch.randn(C, H, W, 2, generator=g) * envelope[None, :, :, None] * gains
    second = kspace + 0.05 * torch.randn(C, H, W, 2, generator=g) * envelope[None, :, :, None] * gains
    image = torch.randn(H, W, generator=g)
    ranged = torch.rand(H, W, generator=g) * 2.0
    constant = torch.full((H, W), 0.7)
    vmin, vmax = 0.25, 1.5

    arrs = {"kspace": kspace.numpy().copy(), "second": second.numpy().copy(), "image": image.numpy().copy(),
            "ranged": ranged.numpy().copy(), "constant": constant.numpy().copy(),
            "ranged_vmin_vmax": np.array([vmin, vmax], dtype=np.float64), "smoothing_factor": np.array(8.0)}
    with tempfile.TemporaryDirectory() as d:
        def run(tag, tensor, **kw):
            mu.save_im(tensor, d, tag + ".png", **kw)
            arr, lo, hi = handed[-1]
            arrs[tag + "/bytes"] = decode_r(os.path.join(d, tag + ".png"))
            arrs[tag + "/handed"] = arr  # float32, as the reference computed it
            norm = matplotlib.colors.Normalize(vmin=lo, vmax=hi)
            arrs[tag + "/normalized"] = np.ma.filled(norm(arr), np.nan).astype(arr.dtype)

        run("kspace_case", kspace.clone(), is_kspace=True)
        run("error_case", second - kspace, is_kspace=True)  # train.py:225: im_recon - k_space
        run("image_case", image.clone())
        run("ranged_case", ranged.clone(), vmin=vmin, vmax=vmax)
        run("constant_case", constant.clone())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mu.stats_per_coil(kspace, C)
    arrs["coil_stats"] = np.array([r[1:] for r in rows_seen[-1]], dtype=np.float64)  # [C,4]: mean, std, max, min
    arrs["coil_stats_text"] = np.array(buf.getvalue())
    arrs["lut"] = matplotlib.colormaps["gray"](np.arange(256), bytes=True)[:, 0].astype(np.uint8)
    arrs["matplotlib_version"] = np.array(matplotlib.__version__)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "display.npz")
    np.savez_compressed(path, **arrs)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
