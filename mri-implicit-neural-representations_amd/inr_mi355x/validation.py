"""Validation epoch of the reference's loops (train.py:199-242, train_kspace_multiscale.py:202-250), shared by the
trainers: predictions -> coil images -> RSS / PSNR / SSIM in the library's kernels (evalchain.image_metrics), the
"best @ epoch" record and the line the reference prints; opt-in, the pictures and the per-coil table the reference writes
next to them (train.py:136-143,221-238), from the same device buffers through the display kernels (display.py)."""
from __future__ import annotations

import os
from typing import Optional

import torch

from .evalchain import ifft2c, image_metrics, metrics_scratch_doubles

# train.py:236-240 (the reference's own spacing, the newline inside included)
VAL_LINE = ("[Validation Epoch: {}/{}] Test loss: {} | Test psnr: {:.4g} | Test ssim: {:.4g} \n Best psnr: {:.4g} @ "
            "epoch {} | Best ssim: {:.4g} @ epoch {}")


def coil_images(flat: torch.Tensor, shape, in_image_space: bool) -> torch.Tensor:
    """[(C*H*W),2] predictions or data -> [C,H,W,2] coil images (ifft2c first in k-space configs, train.py:221-227)."""
    C, H, W = (int(v) for v in shape[:3])
    im = flat.reshape(C, H, W, 2)
    if not in_image_space:
        im = ifft2c(im)
    return im.contiguous()


class ValidationMixin:
    """Best-epoch bookkeeping of train.py:146-149,232-237 (strict '>', 0-based epoch) and the device-side metrics.
    The host class provides self.shape and self.device."""

    def _init_validation(self) -> None:
        self.best_psnr, self.best_psnr_ep = -999999.0, 0
        self.best_ssim, self.best_ssim_ep = -1.0, 0
        self.val_history = []
        self._ref_rss = None
        self._metric_bufs = None
        self._keep_images = False  # enable_validation_images(): keep what the pictures are made of
        self._last_pred = None
        self._display_bufs = None
        self._band_bounds = None  # enable_band_report(): the per-band report of validate() / metrics()
        self._band_dist = None
        self._last_bands = None

    def update_best(self, epoch: int, psnr: float, ssim: float) -> None:
        if psnr > self.best_psnr:
            self.best_psnr, self.best_psnr_ep = psnr, epoch
        if ssim > self.best_ssim:
            self.best_ssim, self.best_ssim_ep = ssim, epoch

    def _device_metrics(self, gt_flat: torch.Tensor, pred_flat: torch.Tensor, in_image_space: bool) -> torch.Tensor:
        """fp64 device vector [psnr, ssim, sse, max_ref, min_ref, max_rec, min_rec, data_range] of the prediction
        against the ground-truth RSS image (computed once, then cached with the output buffers)."""
        C, H, W = (int(v) for v in self.shape[:3])
        if self._metric_bufs is None:
            self._metric_bufs = (torch.empty(H, W, device=self.device),
                                 torch.empty(8, device=self.device, dtype=torch.float64),
                                 torch.empty(max(1, metrics_scratch_doubles(C, H, W)), device=self.device,
                                             dtype=torch.float64))
        if self._ref_rss is None:
            self._ref_rss = image_metrics(None, coil_images(gt_flat, self.shape, in_image_space))[0]
        rss, m, scratch = self._metric_bufs
        image_metrics(self._ref_rss, coil_images(pred_flat, self.shape, in_image_space), rss, m, scratch)
        if self._keep_images:  # the sweep's output; its RSS image stays in the metric buffers
            self._last_pred = pred_flat
        if self._band_bounds is not None:
            self._last_bands = self._band_records(gt_flat, pred_flat)
        return m

    # ---- error by radius (opt-in; nothing below runs unless enable_band_report() was called) ----
    def _default_band_bounds(self):
        """ring_bounds(config['partition']['no_steps']), or 40 rings when the config has no partition"""
        from .bands import ring_bounds
        return ring_bounds(int((getattr(self, "config", {}).get("partition") or {}).get("no_steps", 40)))

    def enable_band_report(self, bounds=None) -> None:
        """From now on validate() / metrics() add 'bands' to their record: bands.band_report of the prediction they score
        against the full data, per band of radius (``bounds``: (lo, hi) pairs, or a number of rings; default: the rings of
        the config's partition) -- and, on undersampled fits, 'bands_sampled' / 'bands_unsampled' for the rows the mask
        kept / dropped.  The parameters and every other record entry stay what they are without it.  More than 64 bands
        (the kernel's limit; a partition of more than 64 rings needs explicit ``bounds``), NaN or lo > hi: ValueError."""
        from .bands import report_bounds
        self._band_bounds = report_bounds(self._default_band_bounds() if bounds is None else bounds)

    def _band_records(self, gt_flat: torch.Tensor, pred_flat: torch.Tensor) -> dict:
        """The report(s) of the sweep ``pred_flat``: one kernel call each, one read-back for all of them."""
        from .bands import band_report, band_stats_many
        if self._band_dist is None:  # once: the radius of every row (the multiscale / ring fits hold it already)
            d = getattr(self, "dist", None)
            self._band_dist = d if d is not None else torch.sqrt(self.coords[:, 1] ** 2 + self.coords[:, 2] ** 2)
        mask = getattr(self, "mask", None)
        names, sel = ["bands"], [(None, 1)]
        if mask is not None:
            names, sel = names + ["bands_sampled", "bands_unsampled"], sel + [(mask, 1), (mask, 0)]
        stats = band_stats_many(self._band_dist, gt_flat, pred_flat, sel, self._band_bounds)
        return {k: band_report(s) for k, s in zip(names, stats)}

    # ---- pictures and per-coil table (opt-in; nothing below runs unless enable_validation_images() was called) ----
    def _display_source(self):
        """(ground-truth rows [(C*H*W),2], in_image_space) of the trainer: what validate() compares against."""
        raise NotImplementedError

    def enable_validation_images(self) -> None:
        """From now on validate() / metrics() keep their prediction (a reference, no copy) for save_validation_images."""
        self._keep_images = True

    def _display(self):
        from . import display as D
        if self._display_bufs is None:
            C, H, W = (int(v) for v in self.shape[:3])
            dev = self.device
            self._display_bufs = dict(
                disp=torch.empty(H, W, device=dev), u8=torch.empty(H, W, device=dev, dtype=torch.uint8),
                stats=torch.empty(C, 4, device=dev, dtype=torch.float64),
                fs=torch.empty(max(D.kspace_display_scratch_floats(C, H, W), D.gray8_scratch_floats(H, W)), device=dev),
                ds=torch.empty(D.coil_stats_scratch_doubles(C, H, W), device=dev, dtype=torch.float64))
        return D, self._display_bufs

    def _write_gray(self, D, b, path: str, img: torch.Tensor, take_abs: bool) -> str:
        D.write_png_gray(path, D.gray8(img, take_abs=take_abs, out=b["u8"], scratch=b["fs"]).cpu())  # H*W bytes cross
        return path

    def _write_kspace(self, D, b, path: str, coils: torch.Tensor, minus: Optional[torch.Tensor] = None) -> str:
        D.kspace_display(coils, minus, out=b["disp"], scratch=b["fs"])
        return self._write_gray(D, b, path, b["disp"], False)

    @torch.no_grad()
    def save_training_images(self, directory: str) -> list:
        """train.py:136-143: train_kspace.png (k-space configs: save_im(..., is_kspace=True) of the full data) and
        train.png (the ground-truth RSS image).  Returns the paths."""
        D, b = self._display()
        gt, in_image_space = self._display_source()
        C, H, W = (int(v) for v in self.shape[:3])
        os.makedirs(directory, exist_ok=True)
        paths = []
        if not in_image_space:
            paths.append(self._write_kspace(D, b, os.path.join(directory, "train_kspace.png"), gt.reshape(C, H, W, 2)))
        if self._ref_rss is None:
            self._ref_rss = image_metrics(None, coil_images(gt, self.shape, in_image_space))[0]
        paths.append(self._write_gray(D, b, os.path.join(directory, "train.png"), self._ref_rss, True))
        return paths

    @torch.no_grad()
    def save_validation_images(self, epoch: int, rec: dict, directory: str, prefix: str = "") -> torch.Tensor:
        """The files of train.py:221-238 for the validation that has just run (0-based ``epoch``; names carry
        epoch + 1 as there): recon_kspace_{e}dB.png and recon_kspace_{e}_error.png (k-space configs only: the prediction,
        and the prediction minus the full data, through save_im's k-space display) and
        recon_{e}_{psnr:.4g}_psnr_{ssim:.4g}_ssim.png (the RSS image validate() scored).  No second sweep: the prediction
        and the RSS image are the ones validate() / metrics() left on the device.  ``rec`` (their record) gains
        'images' (the paths) and 'coil_stats' ([C][mean, std, max, min] of the prediction).  Returns the [C,4] fp64
        statistics on the host.  ``prefix`` goes in front of every file name (the search's 'config_{i}_',
        hp_model_training.py:189-211)."""
        if not self._keep_images or self._last_pred is None:
            raise RuntimeError("save_validation_images: call enable_validation_images() before validate() / metrics()")
        D, b = self._display()
        gt, in_image_space = self._display_source()
        C, H, W = (int(v) for v in self.shape[:3])
        os.makedirs(directory, exist_ok=True)
        pred = self._last_pred.reshape(C, H, W, 2)
        e = epoch + 1
        paths = []
        if not in_image_space:
            paths.append(self._write_kspace(D, b, os.path.join(directory, prefix + "recon_kspace_{}dB.png".format(e)), pred))
            paths.append(self._write_kspace(D, b, os.path.join(directory, prefix + "recon_kspace_{}_error.png".format(e)), pred,
                                            gt.reshape(C, H, W, 2)))
        stats = D.coil_stats(pred, b["stats"], b["ds"]).cpu()  # 32 * C bytes cross
        name = prefix + "recon_{}_{:.4g}_psnr_{:.4g}_ssim.png".format(e, rec["psnr"], rec["ssim"])
        paths.append(self._write_gray(D, b, os.path.join(directory, name), self._metric_bufs[0], True))
        rec["images"] = paths
        rec["coil_stats"] = stats.tolist()
        return stats

    def _finish_validation(self, epoch: int, m: torch.Tensor, loss_sum: Optional[torch.Tensor], n_train_batches: int):
        """The one host read of a validation: PSNR, SSIM and the summed test loss together."""
        parts = [m[:2]] if loss_sum is None else [m[:2], loss_sum.reshape(1)]
        host = torch.cat(parts).cpu().tolist()
        psnr, ssim = float(host[0]), float(host[1])
        # train.py:242: the sum over the VAL batches divided by the TRAIN loader's length
        test_loss = None if loss_sum is None else float(host[2]) / n_train_batches
        self.update_best(epoch, psnr, ssim)
        rec = {"epoch": epoch, "test_loss": test_loss, "psnr": psnr, "ssim": ssim}
        if getattr(self, "coil_compression", None) is not None:  # scored against the K virtual-coil targets
            rec["coil_compression"] = self.coil_compression.summary()
        if getattr(self, "trajectory_info", None) is not None:  # trained on off-grid rows, scored on the grid
            rec["trajectory"] = self.trajectory_info
        if getattr(self, "gridding", None) is not None:  # ... next to the conventional reconstruction of the same samples
            rec["gridding"] = self.gridding
        if getattr(self, "ring_table", None) is not None:  # fitted on ring-normalised targets, scored in the data's units
            rec["ring_normalization"] = self.ring_table.summary()
        if getattr(self, "row_sampling", None) is not None:  # trained on weighted epochs
            rec["row_sampling"] = self._row_sampling_summary()
        if getattr(self, "focal_summary", None) is not None:  # fitted under the focal frequency loss
            rec["focal"] = self.focal_summary
        if self._band_bounds is not None:
            rec.update(self._last_bands)
        self.val_history.append(rec)
        return rec

    def validation_line(self, rec: dict, max_epoch: int) -> str:
        loss = "n/a" if rec["test_loss"] is None else "{:.4g}".format(rec["test_loss"])
        return VAL_LINE.format(rec["epoch"] + 1, max_epoch, loss, rec["psnr"], rec["ssim"], self.best_psnr,
                               self.best_psnr_ep, self.best_ssim, self.best_ssim_ep)
