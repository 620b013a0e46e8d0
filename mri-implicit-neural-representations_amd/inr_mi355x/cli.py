"""The command line the three drivers share (python -m inr_mi355x.train / .train_kspace_multiscale / .train_ring_ensemble):
the parser, the data a fit runs on, the --save-images folders and pictures, and the fit-and-report of the two loops that
have a validation epoch."""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Optional

import torch
import yaml

from .trainer_base import set_default_configs


def get_config(path: str) -> dict:
    """models/utils.py:25-32."""
    if not path:
        return {}
    with open(path, "r") as f:
        return yaml.load(f, Loader=yaml.Loader)


def add_shuffle_flags(ap) -> None:
    ap.add_argument("--shuffle", action="store_true",
                    help="random minibatches: a keyed row permutation per epoch, made on the device (config['shuffle'])")
    ap.add_argument("--shuffle-seed", type=int, default=None,
                    help="key of the permutation (config['shuffle_seed']; default: the trainer's seed)")


def apply_shuffle_flags(config: dict, opts) -> dict:
    if opts.shuffle:
        config["shuffle"] = True
    if opts.shuffle_seed is not None:
        config["shuffle_seed"] = opts.shuffle_seed
    return config


def parse_cli(val_and_samples: bool = True, argv=None, extra_flags=None):
    """(opts, config) of a driver's command line: --config, --output_path, --synthetic, --max_steps, the shuffle flags and
    --save-images; ``val_and_samples``: --val and --data_samples as well (the loops with a validation epoch), and then
    --save-images needs --val.  ``extra_flags(ap)``: a driver's own flags, added before the line is parsed."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True)
    if val_and_samples:
        ap.add_argument("--data_samples", type=str, default="")
    ap.add_argument("--output_path", type=str, default=".")
    ap.add_argument("--synthetic", type=str, default=None,
                    help="C,H,W: fit a synthetic k-space of that shape instead of the scan the config names")
    ap.add_argument("--max_steps", type=int, default=None)
    if val_and_samples:
        ap.add_argument("--val", action="store_true",
                        help="validate every config['val_epoch'] epochs and checkpoint every config['image_save_epoch']")
    add_shuffle_flags(ap)
    ap.add_argument("--save-images", action="store_true",
                    help="with --val: write the reference's pictures to <output_path>/images, checkpoints to "
                         "<output_path>/checkpoints, and print the per-coil table after each validation line")
    from .bands import add_band_report_flag
    add_band_report_flag(ap, "with --val" if val_and_samples else "after the fit")
    from .coils import add_virtual_coils_flag, apply_virtual_coils_flag
    add_virtual_coils_flag(ap)
    from .trajectory import add_baseline_flags, add_trajectory_flag, apply_baseline_flags, apply_trajectory_flag
    add_trajectory_flag(ap)
    add_baseline_flags(ap)
    from .ringnorm import add_ring_normalize_flag
    add_ring_normalize_flag(ap)
    from .sampling import add_row_sampling_flag, apply_row_sampling_flag
    add_row_sampling_flag(ap)
    if extra_flags is not None:
        extra_flags(ap)
    opts = ap.parse_args(argv)
    if val_and_samples and opts.save_images and not opts.val:
        ap.error("--save-images needs --val (the pictures are those of the validation epoch)")
    if opts.band_report is not None and val_and_samples and not opts.val:
        ap.error("--band-report needs --val (the report is made from the validation epoch's prediction)")
    config = apply_virtual_coils_flag(apply_shuffle_flags(set_default_configs(get_config(opts.config)), opts), opts)
    from .ringnorm import apply_ring_normalize_flag
    config = apply_ring_normalize_flag(apply_baseline_flags(apply_trajectory_flag(config, opts), opts), opts)
    return opts, apply_row_sampling_flag(config, opts)


def expand_data_samples(config: dict, samples) -> list:
    """train.py:292-318: ``samples`` = {sample: [slices...]} (the 'samples' entry of the --data_samples YAML) ->
    [(config_i, subdir)], one fit per (sample, slice) with config_i['sample'] / ['slice'] set from the loop (as
    training_script(sample=sample, slice_no=_slice) is called there) and subdir 'sample_{s}_slice_{k}'.  Empty or None:
    the single fit of the config itself, in place ([(config, '')])."""
    if not samples:
        return [(config, "")]
    fits = []
    for sample, slices in samples.items():
        for k in slices:
            cfg = dict(config)
            cfg["sample"], cfg["slice"] = sample, k
            fits.append((cfg, "sample_{}_slice_{}".format(sample, k)))
    return fits


def cli_fits(config: dict, opts):
    """(config_i, opts_i) of every fit a command line asks for: one, or one per (sample, slice) of --data_samples,
    each with its own output folder."""
    samples = (get_config(opts.data_samples) or {}).get("samples") if opts.data_samples else None
    for cfg, sub in expand_data_samples(config, samples):
        o = opts if not sub else argparse.Namespace(**dict(vars(opts), output_path=os.path.join(opts.output_path, sub)))
        yield cfg, o


def cli_data(opts, config: dict, normalization: str, image_space: bool = False):
    """(image, coords, shape) of a fit: --synthetic C,H,W (``normalization``: the default where the config names none),
    or the scan named by config['data_root'/'data'/'set'/'sample'/'slice'] or 'custom_file_or_path' (train.py:271-287,
    train_kspace_multiscale.py:57-72)."""
    return cli_fit_data(opts, config, normalization, image_space)[:3]


def cli_fit_data(opts, config: dict, normalization: str, image_space: bool = False, matrix=None):
    """cli_data plus the coil compression the data came through (None without config['virtual_coils']): (image, coords,
    shape, CoilCompression or None).  With the switch on, --synthetic generates without normalisation, compresses on the
    device (k-space in, k-space out; image space with ``image_space``), then applies datasets.normalize_kspace /
    normalize_image -- compression always comes before normalisation.  ``matrix``: a stored CoilCompression to apply
    instead of computing one (reconstruct --compare)."""
    from .coils import check_virtual_coils
    K = check_virtual_coils(config.get("virtual_coils"))
    if matrix is not None:
        K = matrix.coils_out
    if opts.synthetic:
        from .synthetic import create_coords, make_kspace
        C, H, W = (int(v) for v in opts.synthetic.split(","))
        norm = config.get("normalization", normalization)
        if not K:
            return (*make_kspace(C, H, W, normalization=norm, image_space=image_space), None)
        from .datasets import compress_coils, normalize_image, normalize_kspace
        check_virtual_coils(K, C)  # before anything is generated
        raw = make_kspace(C, H, W, normalization=None, image_space=image_space)[0].reshape(C, H, W, 2).to("cuda")
        data, rec = compress_coils(raw, K, image_space, matrix)
        data = normalize_image(data) if image_space else normalize_kspace(data, norm)
        return data.reshape(K * H * W, 2).contiguous(), create_coords(K, H, W), (K, H, W), rec
    from .datasets import from_config, trainer_inputs
    ds = from_config(config, "cuda", coil_matrix=matrix)
    return (*trainer_inputs(ds), ds.coil_compression)


def cli_folders(tr, opts):
    """(checkpoint folder, image folder or None).  --save-images (train.py:45-46,136-143): the folder tree, then the
    training pictures."""
    os.makedirs(opts.output_path, exist_ok=True)
    if not getattr(opts, "save_images", False):
        return opts.output_path, None
    from .display import prepare_sub_folder
    ckpt_dir, image_dir = prepare_sub_folder(opts.output_path)
    tr.enable_validation_images()
    tr.save_training_images(image_dir)
    if getattr(tr, "gridding", None) is not None:
        tr.save_gridding_image(image_dir)
    if getattr(tr, "cg_sense", None) is not None:  # a calibrated-maps SENSE fit with its CG-SENSE baseline
        tr.save_cg_sense_image(image_dir)
    return ckpt_dir, image_dir


def cli_band_report(tr, opts) -> None:
    """--band-report [N]: validate() / metrics() report the error by radius from now on."""
    from .bands import flag_bounds
    b = flag_bounds(getattr(opts, "band_report", None))
    if b is not None:
        tr.enable_band_report(None if b is True else b)


def print_band_tables(rec: dict) -> None:
    """The table(s) of a record that carries a band report; nothing otherwise."""
    from .bands import REPORT_TITLE, format_band_table
    for key, what in (("bands", ""), ("bands_sampled", ", sampled rows"), ("bands_unsampled", ", unsampled rows")):
        if key in rec:
            print(format_band_table(rec[key], REPORT_TITLE + what), flush=True)


def cli_validation_images(tr, epoch: int, rec: dict, image_dir: str) -> None:
    """The pictures of the validation that has just run, and the per-coil table."""
    from .display import coil_stats_table
    stats = tr.save_validation_images(epoch, rec, image_dir)
    if not tr._display_source()[1]:  # train.py:226: the table belongs to the k-space branch
        print(coil_stats_table(stats), flush=True)


def run_cli(tr, config: dict, opts, extra: Optional[dict] = None) -> None:
    """Fit, then print the JSON result (and, with --val, the reference's validation lines and checkpoints; with
    --save-images, the pictures and the per-coil table as well)."""
    ckpt_dir, image_dir = cli_folders(tr, opts)
    cli_band_report(tr, opts)
    kw = {}
    if opts.val:
        def on_validate(rec):
            print(tr.validation_line(rec, config["max_epoch"]), flush=True)
            print_band_tables(rec)
            if image_dir is not None:
                cli_validation_images(tr, rec["epoch"], rec, image_dir)

        def on_epoch_end(epoch):  # train.py:244-250
            if (epoch + 1) % config["image_save_epoch"] == 0:
                torch.save(tr.checkpoint(), os.path.join(ckpt_dir, "model_%06d.pt" % (epoch + 1)))

        kw = dict(val_epoch=config["val_epoch"], on_validate=on_validate, on_epoch_end=on_epoch_end)
    t0 = time.time()
    tr.fit(opts.max_steps, log_every=config.get("log_iter", 20), **kw)
    torch.cuda.synchronize()
    res = {"steps": tr.global_step, "seconds": time.time() - t0, "psnr": tr.evaluate(),
           "shuffle": tr.shuffle, "shuffle_seed": tr.shuffle_seed if tr.shuffle else None}
    if tr.coil_compression is not None:
        res["coil_compression"] = tr.coil_compression.summary()
    if getattr(tr, "trajectory_info", None) is not None:
        res["trajectory"] = tr.trajectory_info
    if getattr(tr, "gridding", None) is not None:
        res["gridding"] = tr.gridding
    if getattr(tr, "ring_table", None) is not None:
        res["ring_normalization"] = tr.ring_table.summary()
    if getattr(tr, "row_sampling", None) is not None:
        res["row_sampling"] = tr._row_sampling_summary()
    if getattr(tr, "gain_summary", None) is not None:  # a learned-gain fit: exp(-s) over the grid, from evaluate()'s sweep
        res["gain"] = tr.gain_summary
    if getattr(tr, "mixture_summary", None) is not None:  # a mixture-of-heads fit: the gate's weights over the grid
        res["mixture"] = tr.mixture_summary
    if getattr(tr, "sense_summary", None) is not None:  # a SENSE-model fit: its settings and sqrt(sum_c |S_c|^2) over the grid
        res["sense"] = tr.sense_summary
    if getattr(tr, "focal_summary", None) is not None:  # loss 'FFL': the three settings the fit ran under
        res["focal"] = tr.focal_summary
    if extra:
        res.update(extra)
    if opts.val:
        final = tr.metrics()
        res["ssim"] = final["ssim"]
        res.update({k: v for k, v in final.items() if k.startswith("bands")})
        res["validation"] = tr.val_history
        res.update(best_psnr=tr.best_psnr, best_psnr_ep=tr.best_psnr_ep, best_ssim=tr.best_ssim,
                   best_ssim_ep=tr.best_ssim_ep)
    torch.save(tr.checkpoint(), os.path.join(ckpt_dir, "model_%06d.pt" % tr.global_step))
    print(json.dumps(res))
