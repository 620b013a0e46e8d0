"""Multi-scale fitting driver: the loop of the reference's src/train_kspace_multiscale.py:161-201 over
the fused MFN kernel (MultiscaleKFourier, 4 heads) with optional data parallelism over coordinates.

Per step (reference lines 164-195):  outs = model(enc(coords), dist);  loss = 0.1*ConsistencyLoss(outs,
dist) + sum_k 0.5*loss_fn(out_k, gt)  (limit_kspace is a no-op, SURVEY A.4 #2: every head sees the full
gt);  Adam;  per-epoch LambdaLR.  Radii of the nested discs come from the k-means ring partition
(inr_mi355x/clustering.py = the reference's clustering.py; train_kspace_multiscale.py:73-84): pass ``radii`` or
leave it None to have them computed from ``config["partition"]`` (no_steps, no_models).
``config["shuffle"]`` (opt-in): shuffled epochs as in INRTrainer (inr_mi355x/shuffle.py).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .cli import cli_data, cli_fit_data, cli_fits, parse_cli, run_cli  # noqa: F401
from .engine import ConsistencySpec, LossSpec
from .mfn import MultiscaleBoundedFourier, MultiscaleKFourier
from .train import exchange_and_update, wants_sharded_update
from .trainer_base import ResidentFit, mfn_engine


def create_pairs(values: Sequence[float], multiplication_factor: int):
    """train_kspace_multiscale.py:42-47."""
    pairs = [(values[0], values[i + 1]) for i in range(len(values) - 1)]
    return [(p[0], p[1]) for p in pairs for _ in range(multiplication_factor)]


class MultiscaleTrainer(ResidentFit):
    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, dist: torch.Tensor,
                 radii: Optional[Sequence[float]], shape, device, seed: int = 0, rank: int = 0, world: int = 1,
                 process_group=None, mask: Optional[torch.Tensor] = None, mask_seed: Optional[int] = None,
                 coil_compression=None):
        config = self._init_fit(config, shape, device, seed, rank, world, process_group,
                                coil_compression=coil_compression)
        if config.get("loss") == "FFL":  # before the partition below touches the device
            raise NotImplementedError("loss 'FFL' (focal frequency loss) in the multiscale loop: its heads train through "
                                      "the fused multi-head step; FFL fits run in INRTrainer (python -m inr_mi355x.train) only")
        if radii is None:  # train_kspace_multiscale.py:73-84
            from .clustering import partition_and_stats
            C, H, W = int(shape[0]), int(shape[1]), int(shape[2])
            part = config["partition"]
            dev_img = image.to(device).reshape(C, H, W, 2)
            self.mx, radii = partition_and_stats(dev_img, coords.to(device).reshape(C, H, W, 3),
                                                 no_steps=part["no_steps"], no_parts=part["no_models"], stat="max")
            self.mx = torch.cat((self.mx.cpu(), torch.ones(1)))
        self.radii = [float(r) for r in radii]
        kinds = {"L2": (L.LOSS_L2_HALF, 1.0), "L1": (L.LOSS_L1_HALF, 1.0), "LSL": (L.LOSS_LOGSPACE, 0.5)}
        if config["loss"] not in kinds:
            # HDR / FFL / tanh crash in the reference's multiscale script
            raise NotImplementedError(f"loss {config['loss']!r} in the multiscale loop")
        kind, self.scale = kinds[config["loss"]]  # 0.5 * LogSpaceLoss for 'LSL' (train_kspace_multiscale.py:222)
        opts = config.get("loss_opts", {}) or {}
        self.loss = LossSpec(kind, float(opts.get("hdr_eps", 1e-3)), float(opts.get("hdr_ff_sigma", 2.0)),
                             float(opts.get("hdr_ff_factor", 0.5)))
        self._seeded_encoder(seed)  # train_kspace_multiscale.py:90
        if config["model"] == "BoundedFourier":  # train_kspace_multiscale.py:93-95
            self.model = MultiscaleBoundedFourier(config["net"], boundaries=create_pairs(list(radii), 2))
        else:
            self.model = MultiscaleKFourier(config["net"])
        self.model = self.model.to(self.device)
        # ('LogF' / 'none': the filters read encoder.embedding(coords) from memory, train_kspace_multiscale.py:169)
        self.engine, self.enc_B = mfn_engine(self.model, self.encoder, config["encoder"]["embedding"])
        self.sharded_update = wants_sharded_update(config, self.engine.n_params, world)
        if self.sharded_update:
            self.engine.enable_sharded_update(rank, world)
        self.pairs = create_pairs(list(radii), 1)
        self.dist_cpu = dist.reshape(-1).contiguous()
        self._dist_np = self.dist_cpu.detach().cpu().numpy()
        # undersampling / per-coil batches / TV as in the single-scale loop (models/utils.py:102-123;
        # train_kspace_multiscale.py:173-182); in a shuffled fit dist travels with the rows
        self._resident_data(image, coords, config["undersampling"], mask, mask_seed, config["per_coil"],
                            dist=self.dist_cpu.to(self.device))
        self.use_tv = bool(config["use_tv"])  # here TV does not depend on a mask (train_kspace_multiscale.py:173)
        if self.use_tv and not self.per_coil:
            raise ValueError("use_tv needs per_coil batches: tv_loss views the batch as one [H,W,2] coil")
        self._cons = {}  # the consistency term's spec per batch of the unshuffled data, and of the epoch buffers
        self._cons_epoch = []
        self._finish_init()

    def _refilled(self) -> None:
        """Recounts, per batch and disc, the rows outside the disc (the consistency term's mean): one batched op over
        the epoch's dist and one read-back."""
        d = self._t_dist
        rows = []
        if self.pairs[:-1]:
            flags = torch.stack([(d < blo) | (d > bhi) for (blo, bhi) in self.pairs[:-1]])
            rows = self._epoch_buf.batch_sums(flags).tolist()
        self._cons_epoch = [ConsistencySpec(0.1, self.pairs, [1.0 / (2.0 * r[b]) if r[b] else 0.0 for r in rows] + [0.0], 2)
                            for b in range(self._epoch_buf.n_batches)]

    def _cons_spec(self, it: int, lo: int, hi: int) -> ConsistencySpec:
        if self._epoch_buf is not None:
            return self._cons_epoch[it]
        if it not in self._cons:
            # (numpy, not torch: a torch CPU reduction per step leaves its worker threads spinning, which drove the container
            # into its CPU quota -- 87 ms stalls, profiles/r03_config5_steps.txt; here: a first visit of every batch of epoch 0)
            d = self._dist_np[lo:hi]
            inv = []
            for (blo, bhi) in self.pairs[:-1]:
                n_rows = int(np.count_nonzero((d < blo) | (d > bhi)))
                inv.append(1.0 / (2.0 * n_rows) if n_rows else 0.0)  # mse_loss mean over rows x 2 channels
            self._cons[it] = ConsistencySpec(0.1, self.pairs, inv + [0.0], 2)
        return self._cons[it]

    def _tv_step(self, it: int, lo: int, hi: int, count: int) -> torch.Tensor:
        """Per-coil step with TV on the last head (train_kspace_multiscale.py:164-195 with use_tv): forward (stashing)
        -> multi-head loss gradient -> TV gradient added to the last head's -> backward.  Data parallel by image rows
        with a one-row halo, as INRTrainer._tv_step: the halo row only serves the vertical TV pair -- it is masked out
        of the pointwise terms and moved to dist = 0 (inside every disc) for the consistency term."""
        H, W = int(self.shape[1]), int(self.shape[2])

        def image_rows(y0: int, y1: int) -> torch.Tensor:
            ye = min(y1 + 1, H)
            slo, sown, shi = lo + y0 * W, lo + y1 * W, lo + ye * W
            x, d = self._inputs(slo, shi), self.dist[slo:shi]
            outs = self.engine.forward(x, self.enc_B, save=True, dist=d)
            m = torch.ones(shi - slo, dtype=torch.uint8, device=self.device) if self.mask is None else self.mask[slo:shi].clone()
            d_loss = d
            if shi > sown:
                m[sown - slo:] = 0
                d_loss = d.clone()
                d_loss[sown - slo:] = 0
            _, douts = self.engine.loss_grad_multi(self.loss, outs, self.image[slo:shi], count, mask=m, dist=d_loss,
                                                   scale=self.scale, cons=self._cons_spec(it, lo, hi))
            loss = self.engine.tv_grad(outs[-1], douts[-1], y1 - y0, W, H)  # adds to the loss word and to douts[-1]
            self.engine.backward(x, self.enc_B, douts, dist=d)
            return loss

        return self._on_shard(0, H, image_rows)

    def step(self, epoch: int, it: int) -> torch.Tensor:
        if self.shuffle:
            it = self._begin_shuffled(epoch, it)
        lo, hi = self._range(it)
        count = self._count(lo, hi)
        if self.use_tv:
            loss = self._tv_step(it, lo, hi, count)
        else:
            loss = self._on_shard(lo, hi, lambda slo, shi: self.engine.train_step(
                self._inputs(slo, shi, True), self.enc_B, self._t_image[slo:shi], self.loss, count=count,
                mask=None if self.mask is None else self._t_mask[slo:shi], dist=self._t_dist[slo:shi], scale=self.scale,
                cons=self._cons_spec(it, lo, hi)))
        loss = exchange_and_update(self.engine, loss, self.world, self.pg, self.sharded_update, self._lr(epoch),
                                   self.config["beta1"], self.config["beta2"], 1e-8, self.config["weight_decay"])
        self.global_step += 1
        return loss

    def _rebind_encoder(self, enc) -> None:
        super()._rebind_encoder(enc)
        if self.enc_B is not None:
            self.model._enc_B = self.enc_B

    def _forward_chunk(self, lo: int, hi: int) -> torch.Tensor:
        """outs[-1] is the reconstruction (train_kspace_multiscale.py:225)."""
        return self.engine.forward(self._inputs(lo, hi), self.enc_B, save=False, dist=self.dist[lo:hi])[-1]

    @torch.no_grad()
    def validate(self, epoch: int) -> dict:
        """The validation epoch of train_kspace_multiscale.py:202-243, with its quirks: the loop over the heads
        REASSIGNS test_loss, so only the last head's loss survives (:214-224); limit_kspace is a no-op (every head sees
        the full gt); the reconstruction is outs[-1].  Scored by _validated, as INRTrainer.validate."""
        pred = self.predict_all()
        return self._validated(epoch, pred)


def main():
    """CLI with the reference's flags (train_kspace_multiscale.py:50-52): --config, --output_path, --data_samples; the scan
    comes from datasets.py, or a synthetic k-space with --synthetic C,H,W.  --val / --save-images /
    --band-report [N] / --virtual-coils K as inr_mi355x.train."""
    opts, config = parse_cli()
    if config["model"] not in ("BoundedFourier",):
        config["model"] = "MultiscaleKFourier"  # train_kspace_multiscale.py:93-98: anything else is the unbounded net
    for cfg, fit_opts in cli_fits(config, opts):  # one fit, or one per (sample, slice) of --data_samples
        image, coords, shape, cc = cli_fit_data(opts, cfg, "max")
        dist = torch.sqrt(coords[:, 1] ** 2 + coords[:, 2] ** 2)
        tr = MultiscaleTrainer(cfg, image, coords, dist, None, shape, "cuda", coil_compression=cc)
        run_cli(tr, cfg, fit_opts, extra={"radii": tr.radii})


if __name__ == "__main__":
    main()
