"""Validation epoch of the reference's loops (train.py:199-242, train_kspace_multiscale.py:202-250), shared by the
trainers: predictions -> coil images -> RSS / PSNR / SSIM in the library's kernels (evalchain.image_metrics), the
"best @ epoch" record and the line the reference prints."""
from __future__ import annotations

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
        return m

    def _finish_validation(self, epoch: int, m: torch.Tensor, loss_sum: Optional[torch.Tensor], n_train_batches: int):
        """The one host read of a validation: PSNR, SSIM and the summed test loss together."""
        parts = [m[:2]] if loss_sum is None else [m[:2], loss_sum.reshape(1)]
        host = torch.cat(parts).cpu().tolist()
        psnr, ssim = float(host[0]), float(host[1])
        # train.py:242: the sum over the VAL batches divided by the TRAIN loader's length
        test_loss = None if loss_sum is None else float(host[2]) / n_train_batches
        self.update_best(epoch, psnr, ssim)
        rec = {"epoch": epoch, "test_loss": test_loss, "psnr": psnr, "ssim": ssim}
        self.val_history.append(rec)
        return rec

    def validation_line(self, rec: dict, max_epoch: int) -> str:
        loss = "n/a" if rec["test_loss"] is None else "{:.4g}".format(rec["test_loss"])
        return VAL_LINE.format(rec["epoch"] + 1, max_epoch, loss, rec["psnr"], rec["ssim"], self.best_psnr,
                               self.best_psnr_ep, self.best_ssim, self.best_ssim_ep)
