"""Single-scale fitting driver: the loop of the reference's src/train.py:155-251 re-expressed
over the fused MI355X engine (tier 2), with optional data parallelism over coordinates.

Kept from the reference, on purpose: sequential unshuffled batches
(batch i = rows [i*bs,(i+1)*bs) of the C-major grid, last batch short) unless config['shuffle'] asks for the keyed
per-epoch row permutation of inr_mi355x/shuffle.py (opt-in), per-EPOCH LambdaLR
``lr*0.2**min(epoch/max_epoch,1)``, Adam with L2-style weight decay, loss on masked rows only
when undersampled (forward still runs on every row), ``psnr`` with max(x).
Changed, on purpose: inputs stay resident in HBM (no per-step H2D, no per-item DataLoader
collate, no ``.item()`` sync per step), the encoder is fused into layer 0, and unsupported
config values raise instead of falling through.

CLI (same flags as the reference, train.py:255-258):
    python -m inr_mi355x.train --config cfg.yaml [--output_path out] [--synthetic C,H,W] [--val]
                               [--shuffle] [--shuffle-seed S] [--save-images] [--band-report [N]] [--virtual-coils K]
                               [--trajectory ARG] [--trajectory-baseline ARG] [--trajectory-density ARG]
                               [--trajectory-operator ARG] [--ring-normalize ARG] [--data_samples samples.yaml]
--val runs the reference's validation epoch every config['val_epoch'] epochs (its line is printed) and saves a
checkpoint every config['image_save_epoch'] epochs.  --save-images (with --val) also writes the reference's pictures
(train.png, train_kspace.png, recon_kspace_{e}dB.png, recon_kspace_{e}_error.png, recon_{e}_{psnr}_psnr_{ssim}_ssim.png)
to <output_path>/images, moves the checkpoints to <output_path>/checkpoints (models/utils.py:35-44) and prints the
per-coil table after each validation line.  --data_samples names a YAML ``samples: {sample: [slices...]}``: one fit per
(sample, slice) in <output_path>/sample_{s}_slice_{k}/, one JSON line each (train.py:292-318).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib as L
from .cli import (add_shuffle_flags, apply_shuffle_flags, cli_data, cli_fit_data, cli_fits,  # noqa: F401
                  expand_data_samples, get_config, parse_cli, run_cli)
from .engine import LossSpec
from .focal import focal_loss_grad
from .mfn import FourierNet, GaborNet, KGaborNet
from .networks import FFN, SIREN, WIRE, WIRE2D
from .trainer_base import (ResidentFit, hdr_weight, lr_factor, mfn_engine, mlp_engine, run_epochs,  # noqa: F401
                           set_default_configs, shard_rows)

MODELS = {"SIREN": SIREN, "FFN": FFN, "WIRE": WIRE, "WIRE2D": WIRE2D,  # train.py:55-68
          "Fourier": FourierNet, "Gabor": GaborNet, "KGabor": KGaborNet}
MFN_MODELS = ("Fourier", "Gabor", "KGabor")


def allreduce_step_outputs(grads: torch.Tensor, loss: torch.Tensor, world: int, group=None,
                           gbuf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The one exchange step of the data-parallel path: every rank holds the partial
    sums of its contiguous row shard, already divided by the GLOBAL row count, so a plain SUM
    all-reduce (RCCL over xGMI on the GPU box, gloo in the CPU tests) of the flat fp32 gradient and
    of the loss scalar reproduces the single-GPU step up to summation order.  In place on `grads`.
    ``gbuf`` = the engine's [P+1] buffer whose first P words ARE ``grads``: the loss rides in the last word and
    the step costs one collective instead of two (the message is small, so latency is what counts)."""
    if world <= 1:
        return loss
    import torch.distributed as dist
    if gbuf is not None:
        assert gbuf.data_ptr() == grads.data_ptr() and gbuf.numel() == grads.numel() + 1
        if loss.data_ptr() != gbuf[-1:].data_ptr():  # the fused steps already left their loss in that word
            gbuf[-1:].copy_(loss.reshape(1))
        dist.all_reduce(gbuf, op=dist.ReduceOp.SUM, group=group)
        return gbuf[-1].clone()
    dist.all_reduce(grads, op=dist.ReduceOp.SUM, group=group)
    loss = loss.clone()
    dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group)
    return loss


# Below this the replicated update is cheaper than the sharded one's two collectives, chunk copies and re-pack launch:
# measured on one MI355X, Adam + re-pack of BASELINE config 4's 4.47 M parameters is 0.038 ms replicated against 0.039 ms of
# local work per rank sharded 8 ways -- the sharded update starts to pay at several times that size.
SHARDED_UPDATE_MIN_PARAMS = 1 << 24


def wants_sharded_update(config: dict, n_params: int, world: int) -> bool:
    """config["dp_sharded_update"] (True / False; default: networks of >= 2^24 parameters -- none of the BASELINE
    configs) decides between the two exchange steps of exchange_and_update."""
    v = config.get("dp_sharded_update")
    if v is None:
        return world > 1 and n_params >= SHARDED_UPDATE_MIN_PARAMS
    if world <= 1:  # an explicit True on one rank runs the same collectives over a one-rank group (rehearsals of the nccl calls)
        import torch.distributed as dist
        return bool(v) and dist.is_available() and dist.is_initialized()
    return bool(v)


def exchange_and_update(engine, loss: torch.Tensor, world: int, group, sharded: bool, lr: float, beta1: float,
                        beta2: float, eps: float = 1e-8, weight_decay: float = 0.0, l1: float = 0.0,
                        l2: float = 0.0, cplx_reg: Optional[tuple] = None) -> torch.Tensor:
    """Exchange step + optimizer step of one data-parallel iteration (single process in the reference:
    train.py:189-190, train_kspace_multiscale.py:199-200).  Replicated: ONE all-reduce of [gradient | loss], then every
    rank runs the whole Adam update.  Sharded: reduce-scatter, Adam on 1/N of the entries, all-gather, re-pack
    (MLPEngine.adam_step_sharded) -- the same bytes on the links, 1/N of the update per rank.  ``cplx_reg`` = (l1, l2, l2_dir) replaces l1 / l2
    for models with complex64 tensors (INRTrainer._penalty).  Returns the global loss."""
    if sharded:
        if loss.data_ptr() != engine._loss_word.data_ptr():
            engine._loss_word.copy_(loss.reshape(1))
        if cplx_reg is not None:
            return engine.adam_step_sharded(group, lr, beta1, beta2, eps, weight_decay, reg=cplx_reg)
        return engine.adam_step_sharded(group, lr, beta1, beta2, eps, weight_decay, l1, l2)
    loss = allreduce_step_outputs(engine.grads, loss, world, group, engine.gbuf)
    if cplx_reg is not None:  # (l1, l2, l2_dir) of a model with complex tensors: the penalty gradient by inr_reg_grad, once,
        engine.reg_grad(*cplx_reg)  # on the summed gradient (every rank holds the same parameters)
        engine.adam_step(lr, beta1, beta2, eps, weight_decay)
    else:
        engine.adam_step(lr, beta1, beta2, eps, weight_decay, l1, l2)
    return loss


def center_pair_rows(kcoords: torch.Tensor, min_sample: int, n_bands: int = 2):
    """The row pairs of CenterLoss's N_BANDS radial bands (losses.py:176-194), as the reference draws them: band k
    compares dist^2 = ky^2 + kx^2 with the RATIOS (k-1)/N (0.1 for the first band) and k/N; n = min(min_sample, |inner|,
    |ring|); torch.randperm on the default CPU generator, inner set first.  Yields (rows_a, rows_b) int64 on kcoords'
    device; bands with an empty side are skipped."""
    d2 = kcoords[:, 1] ** 2 + kcoords[:, 2] ** 2
    for band in range(1, n_bands + 1):
        r1 = (band - 1) / n_bands or 0.1
        m1 = d2 <= r1
        m2 = (d2 <= band / n_bands) & ~m1
        rows1, rows2 = torch.nonzero(m1)[:, 0], torch.nonzero(m2)[:, 0]
        n = min(min_sample, rows1.numel(), rows2.numel())
        if n == 0:
            continue
        a = torch.randperm(rows1.numel())[:n].to(kcoords.device)
        b = torch.randperm(rows2.numel())[:n].to(kcoords.device)
        yield rows1[a].contiguous(), rows2[b].contiguous()


class INRTrainer(ResidentFit):
    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, shape, device,
                 seed: int = 0, mask: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1,
                 process_group=None, mask_seed: Optional[int] = None, graph_steps: bool = False,
                 model_seed: Optional[int] = None, coil_compression=None):
        config = self._init_fit(config, shape, device, seed, rank, world, process_group, graph_steps, coil_compression,
                                trajectory_ok=True, ring_norm_ok=True, row_sampling_ok=True)
        from .ringnorm import check_ring_normalization
        check_ring_normalization(config, mask)  # refusals, before anything is allocated
        self.in_image_space = bool(config.get("transform", False))
        if self.trajectory is not None:
            self._check_trajectory(config, mask, graph_steps, world)
        if config.get("loss") == "FFL":
            self._check_focal(config, world)
        if config["model"] not in MODELS:
            raise NotImplementedError(f"model {config['model']!r} has no MI355X kernel yet (have {sorted(MODELS)})")
        if config.get("optimizer", "Adam") != "Adam":
            raise NotImplementedError("only Adam (train.py:75-78)")
        self._seeded_encoder(seed, model_seed)
        self.model = MODELS[config["model"]](config["net"]).to(self.device)
        emb = config["encoder"]["embedding"]
        self.is_mfn = config["model"] in MFN_MODELS
        if self.is_mfn and getattr(self.model, "_output_act", False):
            raise NotImplementedError("output_act in the fused training step (no shipped config sets it)")
        if self.is_mfn:
            self.engine, self.enc_B = mfn_engine(self.model, self.encoder, emb)
        else:  # config["precision"]: "f32" (parity path, default) | "bf16" (throughput path)
            self.engine, self.enc_B = mlp_engine(self.model, self.encoder, config["encoder"],
                                                   **{k: config[k] for k in ("precision",) if k in config})
        self.sharded_update = wants_sharded_update(config, self.engine.n_params, world)
        if self.sharded_update:
            self.engine.enable_sharded_update(rank, world)
        self.loss = LossSpec.from_config(config)
        reg = config["regularization"]
        self.l1 = float(reg["strenght"]) if reg["type"] == "L1" else 0.0
        self.l2 = float(reg["strenght"]) if reg["type"] == "L2" else 0.0
        if reg["type"] not in ("none", "L1", "L2"):
            raise NotImplementedError(f"regularization {reg['type']!r}")
        # regularization.py:21-36 on complex64 tensors means sum |z| (L1) and |sum z^2| (L2, a complex square), and
        # model.parameters() includes the frozen omega_0 / scale_0 (networks.py:191-192): the Adam kernel's per-entry sign /
        # 2p terms are the real-parameter forms, so these models take the penalty gradient from inr_reg_grad (_penalty)
        self._cplx_reg = bool(self.l1 or self.l2) and any(c for (_, _, _, c) in self.model._layout)
        if self._cplx_reg:
            P = self.engine.n_params
            sign = torch.ones(P)
            re_idx = []
            for (o, n, _, c) in self.model._layout:
                if c:
                    sign[o + 1:o + n:2] = -1.0
                    re_idx.append(torch.arange(o, o + n, 2))
            self._sq_sign = sign.to(self.device)  # p^2 enters Re(S) with +1 (real entries, real parts) or -1 (imaginary parts)
            self._re_idx = torch.cat(re_idx).to(self.device)
            is_real = torch.ones(P, dtype=torch.bool)
            for (o, n, _, c) in self.model._layout:
                if c:
                    is_real[o:o + n] = False
            self._real_idx = torch.nonzero(is_real)[:, 0].to(self.device)
            frozen = [p.detach().double().cpu() for p in self.model.parameters()
                      if not any(p is q for q in self.model._flat_params)]
            self._frozen_l1 = float(sum(f.abs().sum() for f in frozen))
            self._frozen_l2 = float(sum((f * f).sum() for f in frozen))
        self._resident_data(image, coords, config["undersampling"], mask, mask_seed, config["per_coil"])
        self.use_tv = bool(config["use_tv"]) and self.mask is not None  # train.py:172-175: only inside the mask branch
        if self.use_tv and not self.per_coil:
            raise ValueError("use_tv needs per_coil batches: tv_loss views the batch as one [H,W,2] coil (train.py:175)")
        if self.loss.kind == L.LOSS_CENTER:
            if self.mask is not None:
                # the reference indexes the MASKED predictions with radial masks of the UNMASKED coordinates
                # (train.py:176-179, losses.py:188-189): an IndexError there
                raise NotImplementedError("loss 'LSL' (CenterLoss) with an undersampling mask")
            if self.is_mfn or world > 1 or self.per_coil:
                raise NotImplementedError("loss 'LSL' (CenterLoss): single-rank SIREN / FFN / WIRE fits on plain batches")
        self._hdr_A_train = {}  # the HDR / Center scalar A per batch of the off-grid training rows (config['trajectory'])
        # graph_steps: every batch of the epoch becomes one captured HIP graph (fused kernel, weight-gradient GEMM,
        # reduction, Adam, step advance) replayed from then on -- the batches are fixed views of the resident data
        # (sequential sampler, models/utils.py:126-130), the step count and learning rate live in device memory.
        # Single rank only (the gradient all-reduce sits between the two halves) and only where a step is ONE
        # fused launch sequence on resident views.
        self.graph_steps = bool(graph_steps) and world == 1 and not self.use_tv and \
            self.loss.kind != L.LOSS_CENTER and self.loss.focal is None and (self.enc_B is not None or emb == "none") and not self._cplx_reg
        self._graphs = {}
        # plain single-rank steps of the MLP engines go through inr_train_adam_step (INR_ONE_CALL_STEPS=0: two calls)
        self.one_call_steps = (os.environ.get("INR_ONE_CALL_STEPS", "1") != "0" and not self.is_mfn and not self.use_tv
                               and self.loss.kind != L.LOSS_CENTER and self.loss.focal is None and not self._cplx_reg)
        self._finish_init()

    @staticmethod
    def _check_trajectory(config: dict, mask, graph_steps: bool, world: int) -> None:
        """What an off-grid fit (config['trajectory']) cannot be combined with -- refused before anything
        is allocated."""
        from .undersampling import parse_undersampling_argument
        t = config["trajectory"]
        if config.get("transform", False):
            raise ValueError(f"trajectory = {t!r} with transform: true -- the samples are taken in k-space")
        method = parse_undersampling_argument(config["undersampling"])[0]
        if (method is not None and method.lower() != "none") or mask is not None:
            raise ValueError(f"trajectory = {t!r} with an undersampling pattern or a mask: the trajectory IS the sampling")
        if config["per_coil"] or config["use_tv"]:
            raise ValueError(f"trajectory = {t!r} with per_coil / use_tv: off-grid rows do not form a coil grid")
        if config.get("loss") == "LSL":
            raise NotImplementedError(f"trajectory = {t!r} with loss 'LSL' (CenterLoss)")
        if graph_steps:
            raise NotImplementedError(f"trajectory = {t!r} with graph_steps")
        if world > 1:
            raise NotImplementedError(f"trajectory = {t!r} on more than one rank")

    @staticmethod
    def _check_focal(config: dict, world: int) -> None:
        """What a focal-frequency-loss fit (loss 'FFL') cannot be combined with -- refused before anything
        is allocated.  Masks, shuffled and weighted epochs, trajectories, ring normalisation, virtual coils and the L1 / L2
        penalties only choose rows or targets or act in the Adam kernel: they all apply."""
        if world > 1:
            # n_max is a quantity of the whole batch: a MAX all-reduce would have to sit between the kernel's two passes
            raise NotImplementedError("loss 'FFL' on more than one rank: the batch's largest weight would need an "
                                      "all-reduce between the two passes of inr_focal_loss_grad")
        if config["per_coil"] or config["use_tv"]:
            raise NotImplementedError("loss 'FFL' with per_coil / use_tv: focal-frequency-loss fits train on plain batches")
        if config["model"] in MFN_MODELS:
            raise NotImplementedError(f"loss 'FFL' with model {config['model']!r}: the filter networks' steps are fused "
                                      "around loss_row; FFL fits run SIREN / FFN / WIRE / WIRE2D through the tier-1 calls")
        if config.get("precision", "f32") != "f32":
            raise NotImplementedError(f"loss 'FFL' with precision {config['precision']!r}: the step is the fp32 tier-1 "
                                      "forward, inr_focal_loss_grad and the fp32 backward")

    # ---- one optimizer step on batch `it` of epoch `epoch` --------------------------------------
    def _train_hdr_A(self, it: int, lo: int, hi: int) -> float:
        """A of TRAINING batch ``it``: the grid batch's unless the fit trains on off-grid rows"""
        if self.trajectory is None:
            return self._batch_hdr_A(it, lo, hi)
        if self.loss.kind not in (L.LOSS_HDR, L.LOSS_CENTER):
            return 0.0
        if it not in self._hdr_A_train:
            self._hdr_A_train[it] = float(torch.mean(hdr_weight(self._t_coords[lo:hi], self.loss.sigma)))
        return self._hdr_A_train[it]

    def set_row_weights(self, weights: torch.Tensor) -> None:
        """Weighted epochs (config['row_sampling']): new per-row weights (device fp32 [n_train]) for the
        draws that follow -- the next refill of the epoch buffers, so a caller's ``on_epoch_end`` can steer the next
        epoch by the residual of this one."""
        if self.row_sampling is None:
            raise RuntimeError("set_row_weights: the fit has no config['row_sampling']")
        self._epoch_buf.set_weights(weights)
        self._epoch_buf.mode = "weights"

    def _penalty(self):
        """(value, cplx_reg): the penalty VALUE the reference adds to the logged loss, at the parameters the step starts from
        (train.py:185-192) -- None without a regulariser -- and, for models with complex64 tensors, the (l1, l2, l2_dir)
        that exchange_and_update hands to inr_reg_grad: regularization.py:25-28 is sum |z| over complex entries,
        :34-36 is |S| with S = sum p^2 a complex number (z^2 = a^2 - b^2 + 2iab), over EVERY Parameter, the frozen omega_0 /
        scale_0 included; l2_dir = conj(S) / |S| stays on the device."""
        if not (self.l1 or self.l2):
            return None, None
        p = self.engine.params
        if not self._cplx_reg:
            return (self.l1 * p.abs().sum() if self.l1 else self.l2 * (p * p).sum()), None
        a, b = p[self._re_idx], p[self._re_idx + 1]
        if self.l1:
            return self.l1 * (p[self._real_idx].abs().sum() + torch.hypot(a, b).sum() + self._frozen_l1), (self.l1, 0.0, None)
        s_re = (self._sq_sign * p * p).sum() + self._frozen_l2
        s_im = 2.0 * (a * b).sum()
        mod = torch.hypot(s_re, s_im)
        return self.l2 * mod, (0.0, self.l2, (torch.stack((s_re, -s_im)) / mod).contiguous())

    def step(self, epoch: int, it: int) -> torch.Tensor:
        if self.shuffle:
            it = self._begin_shuffled(epoch, it)
        lo, hi = self._range(it)
        count = self._count(lo, hi)
        A = self._hdr_A_epoch[it] if self._epoch_buf is not None and self._hdr_A_epoch else self._train_hdr_A(it, lo, hi)
        cfg, lr = self.config, self._lr(epoch)
        # the loss the reference logs includes the penalty VALUE at the parameters the step starts from
        # (train.py:185-192); its gradient is formed inside the Adam kernel.  Every rank holds the same parameters.
        penalty, cplx_reg = self._penalty()
        if self.graph_steps:
            loss = self._capture(it, lo, hi, count, A, lr).replay(lr)
        elif self.world == 1 and self.one_call_steps and not self.sharded_update and hi > lo:
            # single rank: nothing sits between the reduction and the update -- one call, one launch less
            m = self._t_mask[lo:hi] if self.mask is not None else None
            loss = self.engine.train_adam_step(self._inputs(lo, hi, True), self.enc_B, self._t_image[lo:hi], self.loss,
                                               lr, count=count, mask=m, hdr_A=A, beta1=cfg["beta1"], beta2=cfg["beta2"],
                                               eps=1e-8, weight_decay=cfg["weight_decay"], l1=self.l1, l2=self.l2)
        else:
            if self.use_tv:
                loss = self._tv_step(lo, count, A)
            elif self.loss.kind == L.LOSS_CENTER:
                loss = self._center_step(lo, hi, A)
            elif self.loss.focal is not None:
                loss = self._focal_step(lo, hi, count)
            else:
                loss = self._on_shard(lo, hi, lambda slo, shi: self._fused(
                    slo, shi, count, self._t_mask[slo:shi] if self.mask is not None else None, A))
            loss = exchange_and_update(self.engine, loss, self.world, self.pg, self.sharded_update, lr, cfg["beta1"],
                                       cfg["beta2"], 1e-8, cfg["weight_decay"], self.l1, self.l2, cplx_reg)
        self.global_step += 1
        return loss if penalty is None else loss + penalty

    def _capture(self, it: int, lo: int, hi: int, count: int, A: float, lr: float):
        """The captured step of batch ``it`` (a fixed view of the resident data), captured on first use and again after
        the engine's workspaces moved."""
        g = self._graphs.get(it)
        if g is None or g.stale:
            cfg = self.config
            m = self.mask[lo:hi] if self.mask is not None else None
            g = self._graphs[it] = self.engine.capture_step(lambda: self._fused(lo, hi, count, m, A), lr, cfg["beta1"],
                                                            cfg["beta2"], 1e-8, cfg["weight_decay"], self.l1, self.l2)
        return g

    def prepare_graphs(self, epoch: int = 0) -> None:
        """Capture every batch of an epoch up front (largest first), so that no capture falls into a timed region.
        Runs each batch's gradient launch once; parameters and the step count do not move."""
        if not self.graph_steps:
            return
        for it in range(self.steps_per_epoch):
            lo, hi = self._range(it)
            self._capture(it, lo, hi, self._count(lo, hi), self._batch_hdr_A(it, lo, hi), self._lr(epoch))

    def _fused(self, slo, shi, count, m, A):
        return self.engine.train_step(self._inputs(slo, shi, True), self.enc_B, self._t_image[slo:shi], self.loss,
                                      count=count, mask=m, hdr_A=A)

    def _center_step(self, lo: int, hi: int, A: float) -> torch.Tensor:
        """CenterLoss ('LSL', train.py:87-88,178-180; losses.py:141-201): forward -> pointwise part -> the random-pair
        term of the two radial bands -> backward.  The pairs are drawn with torch.randperm on the CPU generator in the
        reference's order (band 1: inner, ring; band 2: inner, ring), from masks on dist^2 = ky^2 + kx^2 compared with the
        band RATIOS (losses.py:153-154,180-187).  Single rank, whole batches (pairs span the batch)."""
        x, gt = self._inputs(lo, hi, True), self._t_image[lo:hi]
        out = self.engine.forward(x, self.enc_B, save=True)
        loss, dout = self.engine.loss_grad(self.loss, out, gt, hi - lo, hdr_A=A)
        for rows_a, rows_b in center_pair_rows(self._t_coords[lo:hi], self.loss.min_sample):
            loss = self.engine.center_pairs_grad(out, gt, dout, rows_a, rows_b, 0.1)
        self.engine.backward(x, self.enc_B, dout)
        return loss

    def _focal_step(self, lo: int, hi: int, count: int) -> torch.Tensor:
        """Focal frequency loss ('FFL'): forward (stashing) -> inr_focal_loss_grad on the batch's sampled
        rows (two passes: the batch's largest weight, then the weighted error and its gradient) -> backward.  Single
        rank, whole batches (the weight is relative to the batch's maximum)."""
        x, gt = self._inputs(lo, hi, True), self._t_image[lo:hi]
        m = self._t_mask[lo:hi] if self.mask is not None else None
        out = self.engine.forward(x, self.enc_B, save=True)
        loss, dout = focal_loss_grad(self.loss.focal, out, gt, count, mask=m, loss_out=self.engine._loss)
        self.engine.backward(x, self.enc_B, dout)
        return loss

    def _tv_step(self, lo: int, count: int, A: float) -> torch.Tensor:
        """Per-coil step with total variation (train.py:163-189 with use_tv): forward (stashing) ->
        masked pointwise loss -> TV added on the whole coil grid -> backward.  Data parallel: image rows
        are split over ranks; each rank also evaluates one halo row below its slab so that every vertical
        TV pair is owned by exactly one rank (the halo row's pointwise loss stays with its owner)."""
        H, W = int(self.shape[1]), int(self.shape[2])

        def image_rows(y0: int, y1: int) -> torch.Tensor:
            ye = min(y1 + 1, H)
            slo, shi = lo + y0 * W, lo + ye * W
            out = self.engine.forward(self._inputs(slo, shi), self.enc_B, save=True)
            if self.is_mfn:  # the filter networks' engine hands back [heads = 1, B, out] (train.py:165-169 calls model(coords))
                out = out[0]
            # pointwise loss on the owned rows' sampled coordinates + TV on the grid, one pass (inr_loss_tv_grad)
            loss, dout = self.engine.loss_tv_grad(self.loss, out, self.image[slo:shi], count, y1 - y0, W, H,
                                                  mask=self.mask[slo:shi], hdr_A=A)
            self.engine.backward(self._inputs(slo, shi), self.enc_B, dout.unsqueeze(0) if self.is_mfn else dout)
            return loss

        return self._on_shard(0, H, image_rows)

    # ---- validation (train.py:199-231) -----------------------------------------------------------
    def _forward_chunk(self, lo: int, hi: int) -> torch.Tensor:
        o = self.engine.forward(self._inputs(lo, hi), self.enc_B, save=False)
        return o[0] if self.is_mfn else o

    @torch.no_grad()
    def validate(self, epoch: int) -> dict:
        """The validation epoch of train.py:199-237: a no-grad sweep over every coordinate, scored by _validated."""
        if self.loss.kind == L.LOSS_CENTER:
            # the reference's CenterLoss draws randperm pairs on the CPU generator in the test loss too, which shifts every
            # later training pair; that consumption is not reproduced
            raise NotImplementedError("validation with loss 'LSL' (CenterLoss)")
        return self._validated(epoch, self._predict_raw())

    def load_checkpoint(self, ckpt: dict) -> None:
        if any(k.startswith("scaler.") for k in ckpt.get("net", {})):
            raise ValueError("the checkpoint has 'scaler.' keys: it is a learned-gain fit's -- load it with "
                             "ScaledFitTrainer (python -m inr_mi355x.train_scaling)")
        super().load_checkpoint(ckpt)

    def _rebind_encoder(self, enc) -> None:
        super()._rebind_encoder(enc)
        if self.is_mfn:
            self.model._enc_B = self.enc_B  # the engine (and its Adam state) stays; B is passed per call


def main():
    opts, config = parse_cli()
    for cfg, fit_opts in cli_fits(config, opts):
        image, coords, shape, cc = cli_fit_data(opts, cfg, "coil", image_space=bool(cfg.get("transform", False)))
        run_cli(INRTrainer(cfg, image, coords, shape, "cuda", coil_compression=cc), cfg, fit_opts)


if __name__ == "__main__":
    main()
