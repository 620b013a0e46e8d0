"""What the three fitting drivers share (train.py, train_kspace_multiscale.py, train_ring_ensemble.py): a fit over data
that stays resident in HBM -- undersampling, the training views of a shuffled fit, batch ranges and counts, the epoch
loop, the prediction sweep, validation's test loss, PSNR / SSIM and the checkpoint.  A driver derives from ResidentFit,
builds its model(s) and engine(s) between the set-up calls below and writes its own step(); what differs between the
drivers lives in their hooks, never in a switch here.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .evalchain import image_metrics, psnr, reconstruct
from .networks import Positional_Encoder
from .shuffle import CoilOrder, EpochBuffers, shuffle_settings
from .undersampling import Undersampler, parse_undersampling_argument
from .validation import ValidationMixin, coil_images


def set_default_configs(config: dict) -> dict:
    """utils.py:7-23."""
    config.setdefault("per_coil", False)
    config.setdefault("use_tv", False)
    if "regularization" not in config:
        config["regularization"] = {"type": "none"}
    config.setdefault("undersampling", None)
    config.setdefault("virtual_coils", 0)  # coils.py: K virtual coils instead of the scan's physical ones; 0 = off
    config.setdefault("trajectory", "none")  # trajectory.py: train on off-grid k-space samples; "none" = off
    config.setdefault("trajectory_baseline", "none")  # ... and reconstruct them conventionally too: adjoint | cg-N
    config.setdefault("trajectory_density", None)  # the baseline's density weights; None: ramp (spokes) / uniform (file)
    config.setdefault("trajectory_operator", None)  # the baseline's operator pair: exact | gridding; None: exact, unrecorded
    return config


def hdr_weight(kcoords: torch.Tensor, sigma: float) -> torch.Tensor:
    """(1 - f)^2 per row, f the Gaussian of the k-space radius: the HDR / Center losses' A is its mean over a batch
    (losses.py:241-242,258)."""
    f = torch.exp(-(kcoords[:, 1] ** 2 + kcoords[:, 2] ** 2) / (2 * sigma ** 2))
    return (1 - f) ** 2


def lr_factor(epoch: int, max_epoch: int) -> float:
    """LambdaLR lambda of train.py:153."""
    return 0.2 ** min(epoch / max_epoch, 1)


def shard_rows(lo: int, hi: int, rank: int, world: int):
    """Contiguous split of batch rows [lo,hi) over ranks: rank r gets
    [lo + r*n//world, lo + (r+1)*n//world)."""
    n = hi - lo
    return lo + (rank * n) // world, lo + ((rank + 1) * n) // world


def sampled_prefix(mask_cpu: torch.Tensor) -> np.ndarray:
    """Sampled rows in front of every row of the flattened CPU mask: int64 [n + 1], so that a batch's count is a
    difference of two entries.  (A `mask[lo:hi].sum()` per step is a multi-threaded CPU reduction whose worker threads
    spin on after it: on the GPU boxes that drove the container into its CPU quota -- 87 ms stalls every ~17 steps of the
    per-coil loop, profiles/r03_config5_steps.txt.  A numpy array, not a Python list: 15 coils are 3.5 M entries -- a list
    of ints of that length is > 100 MB.)"""
    cum = np.zeros(mask_cpu.numel() + 1, dtype=np.int64)
    np.cumsum(mask_cpu.flatten().to(torch.int64).numpy(), out=cum[1:])
    return cum


def mfn_engine(model, encoder, embedding: str):
    """(engine, enc_B) of a filter network: 'gauss' is fused into every filter (the model runs on raw coordinates and the
    kernels take the encoder matrix); with 'LogF' / 'none' the filters read encoder.embedding(coords) from memory."""
    if embedding == "gauss":
        model.bind_encoder(encoder)
        return model._engine("gauss"), encoder.B.contiguous()
    return model._engine("x"), None


def mlp_engine(model, encoder, enc_config: dict, **fused):
    """(engine, enc_B) of a SIREN / FFN / WIRE model on the device behind ``encoder`` (``enc_config``: that encoder's
    'embedding' and 'embedding_size'): 'gauss' is fused into layer 0 (raw coordinates in, the kernels take the encoder
    matrix); with 'LogF' / 'none' the first layer reads its input rows from memory.  ``fused``: fused_engine's further
    arguments -- ``precision=config['precision']`` where the key is there and the driver honours it."""
    if enc_config["embedding"] == "gauss":
        return model.fused_engine(enc_config["embedding_size"], **fused), encoder.B.contiguous()
    return model._engine(), None


def _encoded(encoder, enc_B, coords: torch.Tensor) -> torch.Tensor:
    """the rows an engine made by mlp_engine takes for ``coords``: the coordinates themselves where the encoder is fused
    into layer 0, else encoder.embedding's rows ('none': the coordinates again)"""
    return coords if enc_B is not None else encoder.embedding(coords)


def run_epochs(trainer, max_steps, log_every, val_epoch, on_validate, on_epoch_end):
    """Epochs of sequential batches (train.py:155-198, train_kspace_multiscale.py:161-201) with the opt-in validation
    epoch: after the last batch of epoch e when (e + 1) % val_epoch == 0, before the next epoch's learning rate applies."""
    logged = []
    for epoch in range(trainer.config["max_epoch"]):
        for it in range(trainer.steps_per_epoch):
            if max_steps is not None and trainer.global_step >= max_steps:
                return logged
            loss = trainer.step(epoch, it)
            if log_every and trainer.global_step % log_every == 0:
                logged.append((trainer.global_step, trainer._log_value(loss)))
        if val_epoch and (epoch + 1) % val_epoch == 0:
            rec = trainer.validate(epoch)
            if on_validate is not None:
                on_validate(rec)
        if on_epoch_end is not None:
            on_epoch_end(epoch)
    return logged


class ResidentFit(ValidationMixin):
    """A driver's __init__ calls, in this order: _init_fit; (whatever must precede the seed: the k-means partition);
    _seeded_encoder; its model(s) and engine(s); _resident_data; _finish_init.  It provides step(epoch, it),
    _forward_chunk(lo, hi) and, where it trains from epoch buffers, _refilled()."""

    in_image_space = False  # the data are coil images, not k-space (config['transform']): no inverse FFT in validation
    scale = 1.0  # factor on the test loss of validation
    predict_chunk = 1 << 18  # rows per forward call of predict_all

    # ---- set-up ----------------------------------------------------------------------------------
    def _init_fit(self, config: dict, shape, device, seed: int, rank: int, world: int, process_group,
                  graph_steps: bool = False, coil_compression=None, trajectory_ok: bool = False,
                  ring_norm_ok: bool = False, row_sampling_ok: bool = False, step_operator_ok: bool = False) -> dict:
        """Defaults, the shuffle settings (which refuse shuffle with graph steps before anything is allocated), the coil
        compression the data came through (config['virtual_coils'] = K needs the record of a K-coil compression and
        K-coil data, and the other way round: ValueError before anything is allocated), the trajectory of an off-grid fit
        (config['trajectory']; drivers that do not pass ``trajectory_ok`` refuse it), the ring normalisation
        (config['ring_normalization']; drivers that do not pass ``ring_norm_ok`` refuse it), the weighted
        epochs (config['row_sampling']; drivers that do not pass ``row_sampling_ok`` refuse it) and where the
        fit runs.  Returns the trainer's own copy of the config."""
        config = set_default_configs(dict(config))
        self.config = config
        from .ringnorm import check_ring_profile, parse_ring_normalization
        self.ring_norm_spec = parse_ring_normalization(config.get("ring_normalization"))  # no default key: absent = off
        check_ring_profile(config, self.ring_norm_spec)  # config['ring_profile'] belongs to a ring table
        self.ring_table = None
        if self.ring_norm_spec is not None and not ring_norm_ok:
            raise NotImplementedError(f"config['ring_normalization'] = {config['ring_normalization']!r}: ring-normalised "
                                      "fits run in INRTrainer (python -m inr_mi355x.train) only")
        from .trajectory import describe, parse_trajectory
        self.trajectory = parse_trajectory(config["trajectory"])
        if self.trajectory is not None and not trajectory_ok:
            raise NotImplementedError(f"config['trajectory'] = {config['trajectory']!r}: off-grid fits run in INRTrainer "
                                      "(python -m inr_mi355x.train) only")
        self.trajectory_info = describe(self.trajectory, int(shape[1]), int(shape[2]))
        # config['trajectory_baseline'] / ['trajectory_density'] belong to an off-grid fit
        from .trajectory import parse_baseline, parse_density
        self.trajectory_baseline = parse_baseline(config["trajectory_baseline"])
        self.trajectory_density = self.gridding = self.gridding_image = None
        if self.trajectory is None and (self.trajectory_baseline is not None or config["trajectory_density"] is not None):
            raise ValueError(f"config['trajectory_baseline'] = {config['trajectory_baseline']!r} / ['trajectory_density'] = "
                             f"{config['trajectory_density']!r} without config['trajectory']: there are no off-grid "
                             "samples to reconstruct")
        # config['trajectory_operator'] belongs to the baseline; the training samples stay exact.  A driver
        # whose STEP runs the operator pair (off-grid SENSE fits) passes ``step_operator_ok``
        from .trajectory import parse_operator
        self.trajectory_operator = parse_operator(config["trajectory_operator"])
        if self.trajectory_operator is not None and self.trajectory_baseline is None and not step_operator_ok:
            raise ValueError(f"config['trajectory_operator'] = {config['trajectory_operator']!r} without "
                             "config['trajectory_baseline']: it selects the operator inside the baseline only")
        if self.trajectory is not None and (self.trajectory_baseline is not None or config["trajectory_density"] is not None):
            self.trajectory_density = parse_density(config["trajectory_density"], self.trajectory, int(shape[1]),
                                                    int(shape[2]))
        from .coils import check_virtual_coils
        K = check_virtual_coils(config["virtual_coils"])
        if K and coil_compression is None:
            raise ValueError(f"config['virtual_coils'] = {K} but the data ({int(shape[0])} coils) came without a coil "
                             "compression: compress it first (cli.cli_fit_data, datasets.MRIDataset(virtual_coils=K) or "
                             "coils.compress) and pass coil_compression=")
        if coil_compression is not None and (K != coil_compression.coils_out or int(shape[0]) != K):
            raise ValueError(f"config['virtual_coils'] = {K}, the data has {int(shape[0])} coils and the compression "
                             f"record says {coil_compression.coils_in} -> {coil_compression.coils_out}")
        self.coil_compression = coil_compression
        self.shuffle, self.shuffle_seed = shuffle_settings(config, seed, graph_steps)
        from .sampling import check_row_sampling
        self.row_sampling = check_row_sampling(config, self.trajectory, graph_steps, world)  # no default key: absent = off
        if self.row_sampling is not None:
            if not row_sampling_ok:
                raise NotImplementedError(f"config['row_sampling'] = {config['row_sampling']!r}: weighted epochs run in "
                                          "INRTrainer (python -m inr_mi355x.train) only")
            self.shuffle = True  # the fit trains from epoch buffers and the draw always permutes: 'shuffle' adds nothing
        self.device = torch.device(device)
        self.rank, self.world, self.pg = rank, world, process_group
        self.shape = shape
        return config

    def _seeded_encoder(self, seed: int, model_seed: Optional[int] = None) -> None:
        """Construction order and RNG use of train.py:52-71: the seed, then the encoder; the model(s) follow on the same CPU
        generator.  ``model_seed`` (hp_model_training.py:46-49): the search reseeds between the encoder and the model."""
        torch.manual_seed(seed)
        self.encoder = Positional_Encoder(self.config["encoder"], device=self.device)
        if model_seed is not None:
            torch.manual_seed(model_seed)

    def _resident_data(self, image: torch.Tensor, coords: torch.Tensor, undersampling=None,
                       mask: Optional[torch.Tensor] = None, mask_seed: Optional[int] = None, per_coil: bool = False,
                       dist: Optional[torch.Tensor] = None) -> None:
        """Data resident in HBM for the whole fit, and the views the training batches are cut from.
        ``undersampling`` (config['undersampling'], models/utils.py:102-123): train on the zero-filled k-space with the loss
        on sampled rows only; validation still compares with the full k-space (val_loader, utils.py:131-137).  A ``mask``
        given by the caller replaces the drawn one.  ``per_coil``: one batch per coil (MRICoilWrapperDataset,
        nerp_datasets.py:397-441; loader batch_size 1 = one coil, models/utils.py:65-66) so that TV can see a whole coil
        grid.  ``dist`` (device, [n]): a per-row input that travels with the rows."""
        C, H, W = int(self.shape[0]), int(self.shape[1]), int(self.shape[2])
        self.image_full = image.to(self.device).contiguous()
        method, uparams = parse_undersampling_argument(undersampling)
        if mask is None and method is not None and method.lower() != "none":
            masked, _, gm = Undersampler(method, seed=mask_seed).apply(image.reshape(C, H, W, 2).cpu(), uparams)
            image, mask = masked.reshape(-1, 2), gm[:, 0].contiguous()
        self.n = coords.shape[0]
        self.coords = coords.to(self.device).contiguous()
        self.image = self.image_full if mask is None else image.to(self.device).contiguous()
        self.dist = dist
        self.mask_cpu = mask
        self._mask_cum = None if mask is None else sampled_prefix(mask)
        self.mask = mask.to(torch.uint8).to(self.device).contiguous() if mask is not None else None
        self.per_coil = bool(per_coil)
        self.bs = H * W if self.per_coil else int(self.config["batch_size"])
        # config['trajectory']: the training rows are the C*M off-grid samples of the resident k-space (one inr_nudft
        # call); batches, counts and the epoch buffers refer to them, validation keeps reading the grid and the full data
        self.train_coords, self.train_values, self.n_train = self.coords, self.image, self.n
        if self.trajectory is not None:
            from .trajectory import positions, sample_kspace
            values, rows = sample_kspace(self.image_full, self.shape, positions(self.trajectory, H, W))
            self.train_coords, self.train_values = rows.to(self.device).contiguous(), values.contiguous()
            self.n_train = self.train_coords.shape[0]
        self._train_values_data = self.train_values  # the training rows in the data's own units (the gridding baseline's)
        if self.ring_norm_spec is not None:  # before the epoch buffers below are built from train_values
            self._ring_normalize()
        self.steps_per_epoch = math.ceil(self.n_train / self.bs)
        self.global_step = 0
        self._hdr_A = {}  # the HDR / Center scalar A per batch of the unshuffled data, and of the epoch buffers
        self._hdr_A_epoch = []
        # config['shuffle']: plain batches are views of a second set of resident buffers, refilled by one kernel call per
        # epoch (shuffle.EpochBuffers); per-coil batches stay views of the grid and are visited in a permuted order.
        # Validation, predict_all and the test loss keep reading the unshuffled data (the reference's val loader is
        # never shuffled).  Off: the training views ARE the resident data.
        self._epoch_buf = self._coil_order = None
        t = self
        if self.shuffle and self.per_coil:
            self._coil_order = CoilOrder(self.steps_per_epoch, self.shuffle_seed)
        elif self.row_sampling is not None:  # the same buffers, filled by a weighted draw (sampling.py)
            from .sampling import WeightedEpochBuffers, make_weights
            weights = make_weights(self.row_sampling, self.config, self.train_coords, self._train_values_data, self.shape,
                                   self.trajectory)
            t = self._epoch_buf = WeightedEpochBuffers(self.shuffle_seed, self.bs, weights, self.train_coords,
                                                       self.train_values, dist=dist, mask=self.mask, mode=self.row_sampling)
        elif self.shuffle:
            t = self._epoch_buf = EpochBuffers(self.shuffle_seed, self.bs, self.train_coords, self.train_values, dist=dist,
                                               mask=self.mask)
        self._t_coords, self._t_image, self._t_dist, self._t_mask = t.coords, t.image, t.dist, t.mask
        if t is self:
            self._t_coords, self._t_image = self.train_coords, self.train_values

    @torch.no_grad()
    def _ring_normalize(self) -> None:
        """config['ring_normalization']: the table from the rows the fit trains on and from nothing else
        -- the grid rows, or the off-grid samples with the radius of their own coordinates -- and the training targets
        divided by it into a buffer of the trainer's own (train_values; image_full and whatever the caller handed in stay
        what they are).  _norm_full = the normalised full-grid targets of the validation's test loss: the training targets
        themselves on the grid, one more inr_ring_scale call off it."""
        from .ringnorm import make_table
        radius = lambda c: torch.sqrt(c[:, 1] ** 2 + c[:, 2] ** 2).contiguous()
        self._grid_dist = radius(self.coords)
        train_dist = self._grid_dist if self.trajectory is None else radius(self.train_coords)
        self.ring_table = make_table(self.ring_norm_spec, self.config, self.train_values, train_dist)
        self.train_values = self.ring_table.scale(train_dist, self.train_values)  # out of place
        self.ring_table.note_scaled(self.train_values)  # a smooth table's normalized_max
        self._norm_full = self.train_values if self.trajectory is None else \
            self.ring_table.scale(self._grid_dist, self.image_full)

    def _finish_init(self) -> None:
        if "pretrain" in self.config:  # train.py:117-121
            self.load_checkpoint(torch.load(self.config["pretrain"], map_location=self.device))
        self._init_validation()
        if self.trajectory_baseline is not None:
            self._gridding_baseline()

    @torch.no_grad()
    def _gridding_baseline(self) -> None:
        """config['trajectory_baseline']: the conventional reconstruction of the samples the fit trains
        on -- the density-weighted adjoint or N conjugate-gradient iterations (trajectory.cg_baseline) -- made once, scored
        as validation scores the fit (RSS, then PSNR / SSIM against the full data, on the device), with the exact operator
        pair or, under config['trajectory_operator'] = "gridding" (DESIGN.md 4.21), the Kaiser-Bessel pair.  Leaves the record in
        self.gridding and the coil images [C,H,W,2] in self.gridding_image; reads no random numbers and no parameter."""
        import time
        from .trajectory import cg_baseline, positions
        C, H, W = (int(v) for v in self.shape[:3])
        mode, iters = self.trajectory_baseline
        name, w = self.trajectory_density
        torch.cuda.synchronize(self.device)
        t0 = time.time()
        iterates, objective = cg_baseline(self._train_values_data, positions(self.trajectory, H, W), (C, H, W), w, iters,
                                          operator=self.trajectory_operator or "exact")
        self.gridding_image = iterates[-1].contiguous()
        torch.cuda.synchronize(self.device)
        seconds = time.time() - t0
        if self._ref_rss is None:
            self._ref_rss = image_metrics(None, coil_images(self.image_full, self.shape, self.in_image_space))[0]
        self._gridding_rss, m = image_metrics(self._ref_rss, self.gridding_image)[:2]
        psnr_, ssim_ = m[:2].cpu().tolist()
        self.gridding = {"mode": mode, "iters": iters, "density": name, "psnr": psnr_, "ssim": ssim_,
                         "objective": [float(v) for v in objective], "seconds": seconds}
        if self.trajectory_operator is not None:  # the key was given: say which pair made the numbers above
            self.gridding["operator"] = self.trajectory_operator

    @torch.no_grad()
    def save_gridding_image(self, directory: str, prefix: str = "") -> str:
        """gridding_{psnr}_psnr_{ssim}_ssim.png: the baseline's RSS image through the display kernels"""
        if self.gridding is None:
            raise RuntimeError("save_gridding_image: the fit has no config['trajectory_baseline']")
        D, b = self._display()
        os.makedirs(directory, exist_ok=True)
        name = prefix + "gridding_{:.4g}_psnr_{:.4g}_ssim.png".format(self.gridding["psnr"], self.gridding["ssim"])
        return self._write_gray(D, b, os.path.join(directory, name), self._gridding_rss, True)

    # ---- batches ---------------------------------------------------------------------------------
    def _range(self, it: int):
        """rows [lo, hi) of training batch ``it`` (the last batch is short)"""
        return it * self.bs, min((it + 1) * self.bs, self.n_train)

    def _count(self, lo: int, hi: int) -> int:
        """sampled rows of the training batch [lo, hi) (all of them without a mask)"""
        if self._epoch_buf is not None:
            return self._epoch_buf.counts[lo // self.bs]
        return hi - lo if self._mask_cum is None else int(self._mask_cum[hi] - self._mask_cum[lo])

    def _lr(self, epoch: int) -> float:
        return self.config["lr"] * lr_factor(epoch, self.config["max_epoch"])

    def _on_shard(self, lo: int, hi: int, run) -> torch.Tensor:
        """``run(slo, shi)`` on this rank's shard of [lo, hi).  A short last batch (or more ranks than image rows) can leave
        a rank without rows: it contributes zeros to the sum."""
        slo, shi = shard_rows(lo, hi, self.rank, self.world)
        if shi == slo:
            self.engine.grads.zero_()
            return torch.zeros((), device=self.device)
        return run(slo, shi)

    def _begin_shuffled(self, epoch: int, it: int) -> int:
        """Shuffled fits: the batch index step() works with.  Per-coil: the coil visited at position ``it``.  Plain
        batches: ``it`` itself, after the first step of an epoch has refilled the epoch buffers (one kernel call, one
        read-back of the counts) and _refilled() has recomputed what is tied to a batch's contents."""
        if self._coil_order is not None:
            return self._coil_order.at(epoch, it)
        if self._epoch_buf.begin(epoch):
            self._refilled()
        return it

    def _refilled(self) -> None:
        """The epoch buffers hold a new epoch's rows."""
        self._refill_hdr_A()

    def _refill_hdr_A(self) -> None:
        """The HDR / Center scalar A of every batch of the epoch buffers: one batched op over the epoch's coordinates and
        one read-back."""
        if self.loss.kind in (L.LOSS_HDR, L.LOSS_CENTER):
            self._hdr_A_epoch = self._epoch_buf.batch_means(hdr_weight(self._t_coords, self.loss.sigma))

    def _row_sampling_summary(self) -> Optional[dict]:
        return self._epoch_buf.summary() if self.row_sampling is not None else None

    @property
    def focal_summary(self) -> Optional[dict]:
        """{'alpha', 'log_matrix', 'loss_weight'} of a focal-frequency-loss fit (loss 'FFL'); else None"""
        focal = getattr(getattr(self, "loss", None), "focal", None)
        return None if focal is None else focal.summary()

    # ---- the loop --------------------------------------------------------------------------------
    def _log_value(self, loss):
        """what fit() keeps of step()'s return value"""
        return float(loss)

    def fit(self, max_steps: Optional[int] = None, log_every: int = 0, val_epoch: Optional[int] = None,
            on_validate=None, on_epoch_end=None):
        """Runs epochs of sequential batches (train.py:155-198).  Returns the list of losses logged.  ``val_epoch``
        (opt-in): validate() after every val_epoch-th epoch, its record handed to ``on_validate``; ``on_epoch_end(epoch)``
        after every epoch.  Validation reads the parameters only: the trajectory is the same with or without it."""
        return run_epochs(self, max_steps, log_every, val_epoch, on_validate, on_epoch_end)

    # ---- validation (train.py:199-231) -----------------------------------------------------------
    def _forward_chunk(self, lo: int, hi: int) -> torch.Tensor:
        """[hi - lo, 2]: the reconstruction's rows [lo, hi) of the unshuffled data"""
        raise NotImplementedError

    @torch.no_grad()
    def _predict_raw(self, chunk: Optional[int] = None) -> torch.Tensor:
        """the sweep as the network gives it: normalised units in a ring-normalised fit"""
        chunk = chunk or self.predict_chunk
        return torch.cat([self._forward_chunk(lo, min(lo + chunk, self.n)) for lo in range(0, self.n, chunk)], 0)

    @torch.no_grad()
    def predict_all(self, chunk: Optional[int] = None) -> torch.Tensor:
        """[n,2]: the reconstruction of every grid row, in the data's own units"""
        pred = self._predict_raw(chunk)
        if self.ring_table is not None:
            self.ring_table.unscale(self._grid_dist, pred, out=pred)
        return pred

    @torch.no_grad()
    def evaluate(self) -> float:
        ref = reconstruct(self.image_full, self.shape, self.in_image_space)
        return float(psnr(ref, reconstruct(self.predict_all(), self.shape, self.in_image_space)))

    def _inputs(self, lo: int, hi: int, train: bool = False) -> torch.Tensor:
        """the engine's input rows [lo, hi) of the resident data, or of the training views"""
        return _encoded(self.encoder, self.enc_B, (self._t_coords if train else self.coords)[lo:hi])

    def _batch_hdr_A(self, it: int, lo: int, hi: int) -> float:
        """the loss's scalar A of batch ``it`` of the unshuffled data, where the loss has one: A = mean_i((1-f_i)^2) over
        ALL batch coordinates (losses.py:241-242,258)"""
        if self.loss.kind not in (L.LOSS_HDR, L.LOSS_CENTER):
            return 0.0
        if it not in self._hdr_A:
            self._hdr_A[it] = float(torch.mean(hdr_weight(self.coords[lo:hi], self.loss.sigma)))
        return self._hdr_A[it]

    def _validated(self, epoch: int, pred: torch.Tensor) -> dict:
        """Scores the sweep ``pred`` of a validation epoch: the test loss (the config's loss over sequential val batches of
        batch_size rows against the FULL data, times ``scale``, summed, divided by the train loader's length --
        train.py:242), RSS, PSNR and SSIM on the device, one host read.  Updates best_psnr / best_psnr_ep / best_ssim /
        best_ssim_ep (strict '>', 0-based epoch).  Returns {'epoch', 'test_loss', 'psnr', 'ssim'}; test_loss is None for
        per-coil fits (their val batches are not pinned down by the reference: INTEGRATION.md).  Ring-normalised fits:
        ``pred`` is the raw sweep; the test loss compares it with the normalised full-grid targets, then ONE in-place inverse
        inr_ring_scale call takes it to the data's units for everything that follows."""
        loss_sum = None
        targets = self.image_full if self.ring_table is None else self._norm_full
        if not self.per_coil:
            loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
            for it in range(math.ceil(self.n / self.bs)):  # the grid's batches (the training batches, unless off-grid)
                lo, hi = it * self.bs, min((it + 1) * self.bs, self.n)
                if getattr(self.loss, "focal", None) is not None:  # 'FFL': the training step's call, the loss alone
                    from .focal import focal_loss_grad
                    loss, _ = focal_loss_grad(self.loss.focal, pred[lo:hi], targets[lo:hi], hi - lo, want_grad=False,
                                              loss_out=self.engine._loss)
                    loss_sum += loss * self.scale
                    continue
                A = self._batch_hdr_A(it, lo, hi)  # HDR / tanh take the batch's kcoords (train.py:214-217)
                loss, _ = self.engine.loss_grad(self.loss, pred[lo:hi], targets[lo:hi], hi - lo, hdr_A=A)
                loss_sum += loss * self.scale
        if self.ring_table is not None:
            self.ring_table.unscale(self._grid_dist, pred, out=pred)
        m = self._device_metrics(self.image_full, pred, self.in_image_space)
        return self._finish_validation(epoch, m, loss_sum, self.steps_per_epoch)

    def _display_source(self):
        return self.image_full, self.in_image_space

    @torch.no_grad()
    def metrics(self) -> dict:
        """PSNR and SSIM of the current model (validate() without the test loss and the best-epoch record)."""
        m = self._device_metrics(self.image_full, self.predict_all(), self.in_image_space)
        psnr_, ssim_ = m[:2].cpu().tolist()
        rec = {"psnr": psnr_, "ssim": ssim_}
        if self.coil_compression is not None:
            rec["coil_compression"] = self.coil_compression.summary()
        if self.trajectory_info is not None:
            rec["trajectory"] = self.trajectory_info
        if self.gridding is not None:
            rec["gridding"] = self.gridding
        if self.ring_table is not None:
            rec["ring_normalization"] = self.ring_table.summary()
        if self.row_sampling is not None:
            rec["row_sampling"] = self._row_sampling_summary()
        if self.focal_summary is not None:
            rec["focal"] = self.focal_summary
        if self._band_bounds is not None:
            rec.update(self._last_bands)
        return rec

    # ---- checkpoints -----------------------------------------------------------------------------
    def checkpoint(self) -> dict:
        """Same dict as train.py:247-250 ('opt' in torch.optim.Adam.state_dict() layout)."""
        from .checkpoint import save_dict
        ckpt = save_dict(self.model, self.encoder, self.engine, self.config)
        if self.coil_compression is not None:  # the reference's three entries stay as they are
            ckpt["coil_compression"] = self.coil_compression.state()
        if self.ring_table is not None:
            ckpt["ring_normalization"] = self.ring_table.state()
        return ckpt

    def _rebind_encoder(self, enc) -> None:
        """a checkpoint replaced encoder.B: the fused kernels hold their own contiguous copy"""
        if self.enc_B is not None:
            self.enc_B = enc.B.contiguous()

    def _check_same_compression(self, ckpt: dict) -> None:
        """ValueError unless the checkpoint was written under the coil compression the trainer's data came through"""
        from .coils import same_compression
        mine = None if self.coil_compression is None else self.coil_compression.state()
        differs = same_compression(ckpt.get("coil_compression"), mine)
        if differs is not None:
            raise ValueError(f"checkpoint and trainer disagree: {differs} (checkpoint first)")

    def load_checkpoint(self, ckpt: dict) -> None:
        """train.py:117-121 (config['pretrain']): weights, Adam moments / step count and the encoder matrix."""
        from .checkpoint import load_dict
        self._check_same_compression(ckpt)
        from .ringnorm import same_table
        differs = same_table(ckpt.get("ring_normalization"), None if self.ring_table is None else self.ring_table.state())
        if differs is not None:
            raise ValueError(f"checkpoint and trainer disagree: {differs} (checkpoint first)")
        load_dict(self.model, self.encoder, self.engine, ckpt, self._rebind_encoder)
