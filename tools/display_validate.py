#!/usr/bin/env python3
"""One validation epoch with and without its pictures at the headline shape (BASELINE config 2, synthetic 15 x 640 x 368):
wall time of validate() alone and of validate() + save_validation_images(), the host time of the three PNG encodings, and
the bytes that cross device -> host for the pictures and the table (expected 3*H*W + 32*C).

    python tools/display_validate.py [--out FILE] [--reps N]

Under ``rocprofv3 --kernel-trace --stats -- python tools/display_validate.py --reps 1`` the per-kernel times of the
display kernels come from the profiler's kernel statistics."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mri-implicit-neural-representations_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="15,640,368")
    opts = ap.parse_args()
    from inr_mi355x import display as D
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    with open(os.path.join(ROOT, "configs", "config_siren_kspace.yaml")) as f:
        cfg = yaml.safe_load(f)
    C, H, W = (int(v) for v in opts.shape.split(","))
    image, coords, shape = make_kspace(C, H, W, normalization=cfg.get("normalization", "coil"))
    tr = INRTrainer(cfg, image, coords, shape, "cuda")
    tr.enable_validation_images()
    crossed = []
    real_cpu = torch.Tensor.cpu

    def counting_cpu(t, *a, **k):
        if t.is_cuda:
            crossed.append(t.numel() * t.element_size())
        return real_cpu(t, *a, **k)

    with tempfile.TemporaryDirectory() as d:
        tr.save_training_images(d)
        rec = tr.validate(0)  # first call: ground-truth RSS, buffers
        tr.save_validation_images(0, rec, d)  # first call: display buffers, the table's upload
        torch.cuda.synchronize()
        t_val, t_both, t_img, d2h = [], [], [], []
        for e in range(1, opts.reps + 1):
            t0 = time.perf_counter()
            rec = tr.validate(e)
            t1 = time.perf_counter()
            t_val.append(t1 - t0)
            torch.Tensor.cpu = counting_cpu
            del crossed[:]
            try:
                tr.save_validation_images(e, rec, d)
            finally:
                torch.Tensor.cpu = real_cpu
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_img.append(t2 - t1)
            t_both.append(t2 - t0)
            d2h.append(sum(crossed))
        # host share: the three PNG encodings of pictures already on the host
        u8 = [D.read_png_gray(p) for p in rec["images"]]
        t_png = []
        for _ in range(opts.reps):
            t0 = time.perf_counter()
            for k, a in enumerate(u8):
                D.write_png_gray(os.path.join(d, "t%d.png" % k), a)
            t_png.append(time.perf_counter() - t0)
        sizes = [os.path.getsize(p) for p in rec["images"]]
    res = {"shape": [C, H, W], "config": "configs/config_siren_kspace.yaml",
           "validate_ms": 1e3 * min(t_val), "validate_plus_images_ms": 1e3 * min(t_both),
           "save_validation_images_ms": 1e3 * min(t_img), "png_encode_3_files_ms": 1e3 * min(t_png),
           "png_bytes": sizes, "d2h_bytes": d2h[-1], "d2h_bytes_expected": 3 * H * W + 32 * C,
           "psnr": rec["psnr"], "ssim": rec["ssim"]}
    line = json.dumps(res)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
