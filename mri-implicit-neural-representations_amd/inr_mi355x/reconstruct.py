"""Reconstruct from a checkpoint on any grid: the last step of the workflow.

A fitted implicit representation is a continuous function of (coil, y, x); ``Reconstructor`` loads the ``{'net', 'enc'}``
of a ``model_%06d.pt`` checkpoint (the reference's layout, train.py:247-250; one the reference wrote loads too) into the
same encoder, model and engine the trainers build -- without the scan and without Adam moments -- and samples it on the
fit's own grid, a finer or coarser one, a sub-window or a subset of coils.  Coordinates are made on the device a chunk
at a time (inr_mi355x/grid.py): no full coordinate tensor exists at any point.

What the grid means depends on the domain of the fit.  In image-space configs (config['transform']) a finer grid is
super-resolution and a window is a zoom.  In k-space configs a finer grid over the same window samples k-space more
densely, which is a larger field of view after the inverse FFT, and a narrower window keeps the low frequencies only,
which is a lower-resolution image.  A checkpoint of a SENSE-model fit (train_sense.py; 'image.' / 'sens.' keys) holds two
networks in image space: render() gives its coil IMAGES on the grid (a finer one is super-resolution), kspace() their
centred transform, recon.npy holds the images.

CLI:
    python -m inr_mi355x.reconstruct --config C --checkpoint F (--shape C,H,W | --synthetic C,H,W | the config's scan)
        [--scale S] [--height H] [--width W] [--window y0,y1,x0,x1] [--coils 0,3,5]
        [--radii r0,r1,...] [--chunk N] [--compare] [--expand-coils] [--output_path O]
--shape needs no data at all; with --synthetic or the config's scan the shape comes from the data.  --compare adds PSNR
and SSIM against the data (native grid, full window, all coils only).  Prints one JSON line: shape, rows, seconds,
rows_per_s, files (and psnr / ssim with --compare).  Ring-ensemble ``submodel_%d.pt`` files are out of scope: their
radii are not in the file.  A checkpoint of a fit on virtual coils (config['virtual_coils'], coils.py) renders those K coils:
--shape's C must be K, --coils indexes virtual coils, --compare compresses the scan with the matrix stored in the
checkpoint, and --expand-coils also writes recon_physical.npy, the projection on the physical coils.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Optional, Sequence

import numpy as np
import torch

from .grid import GridSpec, grid_rows, resolve_size

MULTISCALE_MODELS = ("MultiscaleKFourier", "BoundedFourier")  # train_kspace_multiscale.py:93-98
FULL_WINDOW = (-1.0, 1.0, -1.0, 1.0)


class Reconstructor:
    """``Reconstructor(config, checkpoint, shape=(C, H, W), device="cuda", radii=None)``: ``config`` is the fit's config
    (dict), ``checkpoint`` the dict a trainer's ``checkpoint()`` returns or the path of a file holding one, ``shape`` the
    fit's own grid.  The single-scale model names are those of train.MODELS; 'MultiscaleKFourier' and 'BoundedFourier'
    need the ``radii`` their trainer reported (ValueError without).  config['precision'] is honoured."""

    predict_chunk = 1 << 18  # rows per forward call of render(), as ResidentFit.predict_chunk

    def __init__(self, config: dict, checkpoint, shape, device="cuda", radii: Optional[Sequence[float]] = None):
        from .networks import Positional_Encoder
        from .train import MFN_MODELS, MODELS
        from .trainer_base import mfn_engine, mlp_engine, set_default_configs
        config = set_default_configs(dict(config))
        self.config = config
        name = config["model"]
        self.multiscale = name in MULTISCALE_MODELS
        if self.multiscale and radii is None:
            raise ValueError(f"model {name!r} needs the radii of its ring partition (the fit's JSON line reports them)")
        if not self.multiscale and name not in MODELS:
            raise NotImplementedError(f"model {name!r} has no MI355X kernel yet (have {sorted(MODELS) + list(MULTISCALE_MODELS)})")
        self.shape = tuple(int(v) for v in shape)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ValueError(f"shape is (C, H, W) of the fit, got {shape!r}")
        self.device = torch.device(device)
        self.in_image_space = bool(config.get("transform", False)) and not self.multiscale
        self.radii = None if radii is None else [float(r) for r in radii]
        emb = config["encoder"]["embedding"]
        with torch.random.fork_rng(devices=[]):  # the initial draws are overwritten by the checkpoint: leave the RNG alone
            self.encoder = Positional_Encoder(config["encoder"], device=self.device)
            if self.multiscale:
                from .mfn import MultiscaleBoundedFourier, MultiscaleKFourier
                from .train_kspace_multiscale import create_pairs
                if name == "BoundedFourier":
                    self.model = MultiscaleBoundedFourier(config["net"], boundaries=create_pairs(self.radii, 2))
                else:
                    self.model = MultiscaleKFourier(config["net"])
            else:
                self.model = MODELS[name](config["net"])
        self.model = self.model.to(self.device)
        self.is_mfn = self.multiscale or name in MFN_MODELS
        self.takes_dist = self.multiscale or name == "KGabor"  # forward(x, dist_to_center) in the reference
        if self.is_mfn:
            self.engine, self.enc_B = mfn_engine(self.model, self.encoder, emb)
        else:
            self.engine, self.enc_B = mlp_engine(self.model, self.encoder, config["encoder"],
                                                   **{k: config[k] for k in ("precision",) if k in config})
        self.engine.drop_training_state()  # forward only: no gradient buffer, no Adam moments
        # a learned-gain fit (train_scaling.py): 'net' holds a ScalerWrapper's keys, and the gain network's
        # size is read from them
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location=self.device)
        self.scaler = self.scaler_engine = None
        from .train_scaling import SCALER_NET, has_scaler_keys
        if has_scaler_keys(checkpoint.get("net", {})):
            if self.is_mfn:
                raise NotImplementedError(f"a checkpoint with 'scaler.' keys and model {name!r}")
            from .networks import FFN
            weights = [v for k, v in checkpoint["net"].items() if k.startswith("scaler.") and k.endswith(".weight")]
            with torch.random.fork_rng(devices=[]):
                self.scaler = FFN(dict(SCALER_NET, network_width=int(weights[0].shape[0]),
                                       network_depth=len(weights))).to(self.device)
            self.scaler_engine = self.scaler._engine()
            self.scaler_engine.drop_training_state()
        # a mixture-of-heads fit (train_multihead.py): 'net' holds 'heads.{k}.' and 'weighted_avg.' keys;
        # self.model / self.engine above are expert 0, the others and the gate (sized from its weights) follow
        self.experts = self.expert_engines = self.gate = self.gate_engine = None
        self.mix_clamp = True
        from .train_multihead import GATE_NET, GATE_PREFIX, has_head_keys, split_state as split_heads
        if has_head_keys(checkpoint.get("net", {})):
            if self.is_mfn:
                raise NotImplementedError(f"a checkpoint with 'heads.' keys and model {name!r}")
            from .networks import FFN
            heads, gate = split_heads(checkpoint["net"])
            weights = [v for k, v in gate.items() if k.endswith(".weight")]
            with torch.random.fork_rng(devices=[]):
                self.experts = [self.model] + [MODELS[name](config["net"]).to(self.device) for _ in heads[1:]]
                self.gate = FFN(dict(GATE_NET, network_output_size=len(heads), network_width=int(weights[0].shape[0]),
                                     network_depth=len(weights))).to(self.device)
            self.expert_engines = [self.engine]
            for m in self.experts[1:]:
                eng = mlp_engine(m, self.encoder, config["encoder"])[0]
                eng.drop_training_state()
                self.expert_engines.append(eng)
            self.gate_engine = self.gate._engine()
            self.gate_engine.drop_training_state()
            self.mix_clamp = bool((checkpoint.get("mixture") or {}).get("clamp", True))
        # a SENSE-model fit (train_sense.py): 'net' holds 'image.' and 'sens.' keys; self.model /
        # self.engine above are the image network, the sensitivity network (sized from its weights) and its encoder
        # follow.  Both networks live in image space: render() gives coil IMAGES (renders_images) although the fit's data
        # are k-space (in_image_space stays what the config says), kspace() their centred transform
        self.sens_model = self.sens_engine = self.sens_encoder = self.sens_enc_B = self.sense_scale = None
        # ... or, fitted on calibrated maps, 'image.' keys alone and the windowed centre block of
        # k-space in 'sense': the maps are rebuilt for every rendered grid (inr_sense_lowres, inr_sense_maps)
        self.sense_block = self.sense_calib = None
        self._sense_maps = {}
        self.renders_images = self.in_image_space  # what render() returns; in_image_space: what the fit's DATA are
        from .sense import has_sense_keys, sens_encoder_config, split_state as split_sense
        if has_sense_keys(checkpoint.get("net", {})):
            if self.is_mfn:
                raise NotImplementedError(f"a checkpoint with 'image.' / 'sens.' keys and model {name!r}")
            meta = checkpoint.get("sense")
            if meta is None:
                raise ValueError("a checkpoint with 'image.' / 'sens.' keys carries a 'sense' entry (the factor of the "
                                 "product and the sensitivity encoder); this one has none")
        if has_sense_keys(checkpoint.get("net", {})) and meta.get("maps", "learned") == "calibrated":
            if meta.get("block") is None or meta.get("calib") is None:
                raise ValueError("a calibrated-maps checkpoint carries sense['block'] and sense['calib']; this one does not")
            self.sense_block = meta["block"].to(self.device, torch.float32).contiguous()
            if self.sense_block.dim() != 4 or self.sense_block.shape[0] != self.shape[0]:
                raise ValueError(f"sense['block'] has shape {tuple(self.sense_block.shape)}, the fit {self.shape[0]} coils")
            self.sense_calib = dict(meta["calib"])
            self.sense_scale = float(meta["scale"])
            self.renders_images = True
            self.sense_group = max(1, int(meta.get("coils_per_step") or self.shape[0]))
        elif has_sense_keys(checkpoint.get("net", {})):
            from .networks import FFN
            weights = [v for k, v in split_sense(checkpoint["net"])[1].items() if k.endswith(".weight")]
            sens_enc = sens_encoder_config(meta, config["encoder"])
            with torch.random.fork_rng(devices=[]):
                self.sens_encoder = Positional_Encoder(sens_enc, device=self.device)
                self.sens_model = FFN({"network_input_size": int(weights[0].shape[1]), "network_output_size": 2,
                                       "network_width": int(weights[0].shape[0]),
                                       "network_depth": len(weights)}).to(self.device)
            self.sens_engine, self.sens_enc_B = mlp_engine(self.sens_model, self.sens_encoder, sens_enc)
            self.sens_engine.drop_training_state()
            self.sense_scale = float(meta["scale"])
            self.renders_images = True
            # coils per forward sweep and per transform: the trainer's groups, so that the native grid gives its bits
            self.sense_group = max(1, int(meta.get("coils_per_step") or self.shape[0]))
        self.load(checkpoint)
        self._bufs = None
        self._metric_bufs = {}

    # ---- the checkpoint --------------------------------------------------------------------------
    def _rebind_encoder(self, enc) -> None:
        """the checkpoint replaced encoder.B: the fused kernels hold their own contiguous copy (ResidentFit._rebind_encoder)"""
        if self.enc_B is not None:
            self.enc_B = enc.B.contiguous()
            if self.is_mfn:
                self.model._enc_B = self.enc_B

    def _rebind_sens_encoder(self, enc) -> None:
        if self.sens_enc_B is not None:
            self.sens_enc_B = enc.B.contiguous()

    def _parts(self):
        """the part list of the trainer that wrote the checkpoint, over this Reconstructor's networks"""
        from .checkpoint import Part
        from .sense import IMAGE_PREFIX, SENS_PREFIX
        from .train_multihead import GATE_PREFIX, HEAD_PREFIX
        from .train_scaling import PREFIXES
        first = (self.model, self.engine, self.encoder, self._rebind_encoder)
        if self.experts is not None:
            heads = [Part(f"{HEAD_PREFIX}{k}.", m, e) for k, (m, e) in enumerate(zip(self.experts, self.expert_engines))]
            heads[0] = Part(heads[0].prefix, *first)  # the encoder travels with expert 0
            return heads + [Part(GATE_PREFIX, self.gate, self.gate_engine)]
        if self.sens_model is not None:
            return [Part(IMAGE_PREFIX, *first),
                    Part(SENS_PREFIX, self.sens_model, self.sens_engine, self.sens_encoder, self._rebind_sens_encoder)]
        if self.scaler is not None:
            return [Part(PREFIXES[0], *first), Part(PREFIXES[1], self.scaler, self.scaler_engine)]
        return [Part(IMAGE_PREFIX if self.sense_block is not None else "", *first)]

    def load(self, checkpoint) -> None:
        """ckpt['net'] and ckpt['enc'] (checkpoint.load_weights); ckpt['opt'] is not read."""
        from .checkpoint import load_parts
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location=self.device)
        if "net" not in checkpoint:
            raise ValueError("not a {'net', 'enc', 'opt'} checkpoint (ring-ensemble submodel files are not supported)")
        self.coil_compression = None  # coils.CoilCompression of a fit on virtual coils: render() gives those K coils
        if checkpoint.get("coil_compression") is not None:
            from .coils import CoilCompression
            self.coil_compression = CoilCompression.from_state(checkpoint["coil_compression"])
            if self.shape[0] != self.coil_compression.coils_out:
                raise ValueError(f"the checkpoint was fitted on {self.coil_compression.coils_out} virtual coils (of "
                                 f"{self.coil_compression.coils_in} physical ones) but shape has C = {self.shape[0]}")
        self.ring_table = None  # ringnorm.RingTable of a ring-normalised fit: render() un-scales every chunk with it
        if checkpoint.get("ring_normalization") is not None:
            from .ringnorm import RingTable
            self.ring_table = RingTable.from_state(checkpoint["ring_normalization"])
        net, encs = checkpoint["net"], [checkpoint.get("enc")]
        if self.experts is not None:
            from .train_multihead import split_state as split_heads
            heads, gate = split_heads(net)
            if len(heads) != len(self.experts):
                raise ValueError(f"the checkpoint has {len(heads)} heads, this Reconstructor {len(self.experts)}")
            nets = heads + [gate]
        elif self.sense_block is not None:
            from .sense_calib import image_net_of
            nets = [image_net_of(net)]
        elif self.sens_model is not None:
            from .sense import split_state as split_sense
            nets, encs = split_sense(net), encs + [checkpoint["sense"].get("enc_B")]
        elif self.scaler is not None:
            from .train_scaling import split_state
            nets = split_state(net)
        else:
            nets = [net]
        load_parts(self._parts(), nets, encs + [None] * (len(nets) - len(encs)), None, weights_only=True)

    @torch.no_grad()
    def expand(self, pred: torch.Tensor) -> torch.Tensor:
        """[coils_in, H', W', 2]: the physical-coil projection of a rendering of ALL virtual coils (inr_coil_apply with the
        conjugate transpose of the stored matrix)."""
        if self.coil_compression is None:
            raise ValueError("the checkpoint carries no coil compression: there is nothing to expand")
        if pred.dim() != 4 or pred.shape[0] != self.coil_compression.coils_out:
            raise ValueError(f"expand() takes all {self.coil_compression.coils_out} virtual coils, got {tuple(pred.shape)}")
        return self.coil_compression.expand(pred.contiguous())

    # ---- sampling --------------------------------------------------------------------------------
    def grid(self, height: Optional[int] = None, width: Optional[int] = None, scale: Optional[float] = None,
             window: Optional[Sequence[float]] = None, coils: Optional[Sequence[int]] = None) -> GridSpec:
        """The grid render() samples: grid.resolve_size's resolution rule on the fit's H x W, the window (default: the
        fit's own, -1, 1, -1, 1) and the coils (default: all)."""
        C, H, W = self.shape
        h, w = resolve_size(H, W, height, width, scale)
        return GridSpec(C, h, w, coils=coils, window=FULL_WINDOW if window is None else window)

    def _forward_rows(self, coords: torch.Tensor, dist: Optional[torch.Tensor]) -> torch.Tensor:
        """[n,2]: the forward call of the trainers' _forward_chunk on these coordinates"""
        from .trainer_base import _encoded
        x = _encoded(self.encoder, self.enc_B, coords)  # LogF: the filters / first layer read the encoded rows
        if self.is_mfn:
            o = self.engine.forward(x, self.enc_B, save=False, dist=dist if self.takes_dist else None)
            return o[-1]  # the last head is the reconstruction (train_kspace_multiscale.py:225); single-scale: the only one
        if self.experts is not None:  # z as below; the trainers' mix_apply over the K experts' rows
            ys = [eng.forward(x, self.enc_B, save=False) for eng in self.expert_engines]
            z = torch.stack((coords[:, 0], dist), dim=1).contiguous()
            from .mix import mix_apply
            return mix_apply(ys, self.gate_engine.forward(z, None, save=False), clamp=self.mix_clamp, out=ys[0])
        y = self.engine.forward(x, self.enc_B, save=False)
        if self.scaler is not None:  # z = (coil column, the radius the grid kernel made), as gain.gain_inputs
            z = torch.stack((coords[:, 0], dist), dim=1).contiguous()
            s = self.scaler_engine.forward(z, None, save=False).view(-1)
            from .gain import gain_apply
            return gain_apply(y, s, out=y)
        return y

    @torch.no_grad()
    def render(self, height: Optional[int] = None, width: Optional[int] = None, scale: Optional[float] = None,
               window: Optional[Sequence[float]] = None, coils: Optional[Sequence[int]] = None,
               chunk: Optional[int] = None) -> torch.Tensor:
        """[C', H', W', 2] fp32 on the device.  ``scale`` multiplies H and W (rounded to the nearest integer, never below
        1), ``height`` / ``width`` override it; ``window`` = (y0, y1, x0, x1) inside or outside the fit's -1, 1, -1, 1;
        ``coils`` = which coils, in output order.  Image-space configs: a finer grid is super-resolution, a window a zoom.
        k-space configs: a finer grid over the same window is a larger field of view, a narrower window a lower-resolution
        image.  Per ``chunk`` rows: the grid kernel into two reused buffers, the trainers' forward call, a slice of the
        output; no full coordinate tensor is made.  A checkpoint of a ring-normalised fit: every chunk is
        taken back to the data's units by one in-place inr_ring_scale call with the radius the grid kernel made."""
        spec = self.grid(height, width, scale, window, coils)
        n = spec.rows
        chunk = int(chunk or self.predict_chunk)
        if chunk < 1:
            raise ValueError(f"chunk = {chunk}")
        chunk = min(chunk, n)
        if self._bufs is None or self._bufs[0].shape[0] < chunk:
            self._bufs = (torch.empty(chunk, 3, device=self.device), torch.empty(chunk, device=self.device))
        cbuf, dbuf = self._bufs
        if self.sens_model is not None or self.sense_block is not None:
            return self._render_sense(spec, chunk, cbuf)
        out = torch.empty(n, 2, device=self.device)
        with_dist = self.takes_dist or self.ring_table is not None or self.scaler is not None or \
            self.experts is not None
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            c, d = grid_rows(spec, lo, hi, coords_out=cbuf[:hi - lo], dist_out=dbuf[:hi - lo] if with_dist else None,
                             with_dist=with_dist)
            out[lo:hi] = self._forward_rows(c, d)
            if self.ring_table is not None:
                self.ring_table.unscale(d, out[lo:hi], out=out[lo:hi])
        return out.reshape(*spec.shape, 2)

    def _render_sense(self, spec: GridSpec, chunk: int, cbuf: torch.Tensor) -> torch.Tensor:
        """A SENSE-model checkpoint: coil IMAGES [C', H', W', 2] = scale * S_c * I on the grid, straight from
        inr_sense_apply(shift = 0) -- the image network on the (y, x) rows of one plane with the coil column set to 0,
        the sensitivity network on every row, in chunks of rows as the trainer's sweep.  Both networks live in image
        space, so a finer grid is genuine super-resolution.  kspace() gives the centred transform where it is wanted."""
        from .sense import sense_apply
        from .trainer_base import _encoded
        n_coils, h, w = spec.shape

        def sweep(engine, encoder, enc_B, grid, zero_coil):
            out = torch.empty(grid.rows, 2, device=self.device)
            for lo in range(0, grid.rows, chunk):
                hi = min(lo + chunk, grid.rows)
                c = grid_rows(grid, lo, hi, coords_out=cbuf[:hi - lo], with_dist=False)[0]
                if zero_coil:
                    c[:, 0] = 0.0
                out[lo:hi] = engine.forward(_encoded(encoder, enc_B, c), enc_B, save=False)
            return out

        plane = GridSpec(spec.coils_total, h, w, coils=spec.coils[:1], window=spec.window)
        img = sweep(self.engine, self.encoder, self.enc_B, plane, True)
        out = torch.empty(n_coils, h, w, 2, device=self.device)
        if self.sense_block is not None:  # calibrated maps: all coils' maps on this grid (the RSS is over every coil)
            maps = self._calibrated_maps(h, w, spec.window)
            for c0 in range(0, n_coils, self.sense_group):
                c1 = min(c0 + self.sense_group, n_coils)
                sens = maps[list(spec.coils[c0:c1])].reshape(-1, 2).contiguous()
                sense_apply(img, sens, c1 - c0, h, w, self.sense_scale, 0, out=out[c0:c1])
            return out
        for c0 in range(0, n_coils, self.sense_group):  # the trainer's coil groups: one group's sensitivities at a time
            c1 = min(c0 + self.sense_group, n_coils)
            group = GridSpec(spec.coils_total, h, w, coils=spec.coils[c0:c1], window=spec.window)
            sens = sweep(self.sens_engine, self.sens_encoder, self.sens_enc_B, group, False)
            sense_apply(img, sens, c1 - c0, h, w, self.sense_scale, 0, out=out[c0:c1])
        return out

    def _calibrated_maps(self, h: int, w: int, window) -> torch.Tensor:
        """[C,h*w,2]: the calibrated maps on a grid, rebuilt from the stored block (the last grid is kept)"""
        from .sense_calib import calibrate
        key = (int(h), int(w), tuple(float(v) for v in window))
        if key not in self._sense_maps:
            _, H, W = self.shape
            self._sense_maps = {key: calibrate(self.sense_block, H, W, float(self.sense_calib["floor"]), h, w, key[2])[0]}
        return self._sense_maps[key]

    @torch.no_grad()
    def kspace(self, pred: torch.Tensor) -> torch.Tensor:
        """[C', H', W', 2]: the k-space of a rendering -- the rendering itself for a k-space fit, evalchain.fft2c of the
        coil images for an image-space one (config['transform'], or a SENSE-model checkpoint, whose k-space on the native
        grid equals the trainer's predict_all() bit for bit)."""
        from .evalchain import fft2c
        if pred.dim() != 4 or pred.shape[-1] != 2:
            raise RuntimeError(f"pred has shape {tuple(pred.shape)}, expected [C,H,W,2]")
        if not self.renders_images:
            return pred.contiguous()
        if self.sens_model is None and self.sense_block is None:
            return fft2c(pred).contiguous()
        g = self.sense_group  # transformed in the trainer's coil groups, as the sweep
        return torch.cat([fft2c(pred[c:c + g]) for c in range(0, pred.shape[0], g)], 0).contiguous()

    # ---- pictures and numbers --------------------------------------------------------------------
    def _coil_images(self, pred: torch.Tensor) -> torch.Tensor:
        from .evalchain import ifft2c
        if pred.dim() != 4 or pred.shape[-1] != 2:
            raise RuntimeError(f"pred has shape {tuple(pred.shape)}, expected [C,H,W,2]")
        return (pred if self.renders_images else ifft2c(pred)).contiguous()

    @torch.no_grad()
    def rss(self, pred: torch.Tensor) -> torch.Tensor:
        """[H', W']: the root-sum-of-squares image of a prediction -- ifft2c first unless config['transform'], then
        inr_image_metrics without a reference (the kernel of the validation epoch)."""
        from .evalchain import image_metrics
        return image_metrics(None, self._coil_images(pred))[0]

    @torch.no_grad()
    def compare(self, pred: torch.Tensor, image_full: torch.Tensor, bands=None) -> dict:
        """{'psnr', 'ssim'} of a prediction on the fit's own full grid against the data ``image_full`` [(C*H*W),2] (or
        [C,H,W,2]), through the kernel validate() scores with.  ``bands`` ((lo, hi) pairs, a number of rings, or True for
        the rings of the config's partition / 40): adds 'bands', bands.band_report of the prediction against the data per
        band of the grid's own radius (grid.grid_rows' dist)."""
        from .evalchain import image_metrics
        C, H, W = self.shape
        if tuple(pred.shape) != (C, H, W, 2):
            raise ValueError(f"compare() takes a prediction on the fit's own grid {(C, H, W, 2)}, got {tuple(pred.shape)}")
        data = image_full.to(self.device).reshape(C, H, W, 2)
        from .evalchain import ifft2c
        ref = image_metrics(None, (data if self.in_image_space else ifft2c(data)).contiguous())[0]  # the DATA's domain
        m = image_metrics(ref, self._coil_images(pred))[1]
        psnr, ssim = m[:2].cpu().tolist()
        out = {"psnr": psnr, "ssim": ssim}
        if bands is not None:
            from .bands import band_report, band_stats, report_bounds
            from .grid import GridSpec, grid_rows
            steps = int((self.config.get("partition") or {}).get("no_steps", 40))
            dist = grid_rows(GridSpec(C, H, W), 0, C * H * W, with_dist=True, device=self.device)[1]
            if not self.in_image_space:  # k-space data: compare in k-space, whatever render() returns
                pred = self.kspace(pred)
            out["bands"] = band_report(band_stats(dist, image_full.to(self.device).reshape(-1, 2), pred.reshape(-1, 2),
                                                  bounds=report_bounds(bands, steps)))
        return out

    @torch.no_grad()
    def save(self, directory: str, pred: torch.Tensor) -> list:
        """Writes recon.npy (the prediction), recon.png (its RSS image through inr_gray8) and, for k-space configs,
        recon_kspace.png (inr_kspace_display of the prediction, as the validation epoch's recon_kspace picture).
        Returns the paths."""
        from . import display as D
        os.makedirs(directory, exist_ok=True)
        paths = [os.path.join(directory, "recon.npy")]
        np.save(paths[0], pred.detach().cpu().numpy())
        paths.append(os.path.join(directory, "recon.png"))
        D.write_png_gray(paths[-1], D.gray8(self.rss(pred), take_abs=True).cpu())
        if not self.in_image_space:  # (where render() gives images of a k-space fit: their transform)
            paths.append(os.path.join(directory, "recon_kspace.png"))
            D.write_png_gray(paths[-1], D.gray8(D.kspace_display(self.kspace(pred))).cpu())
        return paths


# ---- command line ------------------------------------------------------------------------------------------------------
def _numbers(kind, count: Optional[int], what: str):
    def parse(text: str):
        try:
            vals = [kind(v) for v in text.split(",")]
        except ValueError:
            raise argparse.ArgumentTypeError(f"{what}: {text!r} is not a comma-separated list of {kind.__name__} values")
        if not vals or (count is not None and len(vals) != count):
            raise argparse.ArgumentTypeError(f"{what}: expected {count if count is not None else 'at least one'} "
                                             f"value(s), got {text!r}")
        return vals
    return parse


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m inr_mi355x.reconstruct",
                                 description="Sample a fitted model from its checkpoint on any grid.")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--shape", type=_numbers(int, 3, "--shape C,H,W"), default=None,
                    help="C,H,W of the fit: no data is read at all")
    ap.add_argument("--synthetic", type=_numbers(int, 3, "--synthetic C,H,W"), default=None,
                    help="C,H,W: the synthetic k-space the training command's --synthetic made")
    ap.add_argument("--scale", type=float, default=None, help="multiplies H and W (rounded, never below 1)")
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--window", type=_numbers(float, 4, "--window y0,y1,x0,x1"), default=None,
                    help="y0,y1,x0,x1; the fit's own grid is -1,1,-1,1")
    ap.add_argument("--coils", type=_numbers(int, None, "--coils"), default=None,
                    help="coil indices, in output order (virtual coils for a checkpoint that carries coil compression)")
    ap.add_argument("--expand-coils", action="store_true",
                    help="a checkpoint fitted on virtual coils: also write the physical-coil projection (recon_physical.npy)")
    ap.add_argument("--radii", type=_numbers(float, None, "--radii"), default=None,
                    help="ring radii of a multiscale fit (its training command's JSON line)")
    ap.add_argument("--chunk", type=int, default=None, help="rows per forward call")
    ap.add_argument("--compare", action="store_true", help="PSNR / SSIM against the data (native grid only)")
    ap.add_argument("--output_path", type=str, default=".")
    from .bands import add_band_report_flag
    add_band_report_flag(ap, "with --compare")
    return ap


def parse_args(argv=None):
    """The command line, with the argument errors that need no GPU: --shape with --synthetic, --compare without data or
    off the fit's own full grid, sizes below 1."""
    import sys
    ap = build_parser()
    argv, joined = list(sys.argv[1:] if argv is None else argv), []
    while argv:  # "--window -0.5,0.25,0.1,0.7": argparse would take the list, which starts with '-', for an option
        a = argv.pop(0)
        joined.append(a + "=" + argv.pop(0) if a == "--window" and argv else a)
    opts = ap.parse_args(joined)
    if opts.shape is not None and opts.synthetic is not None:
        ap.error("--shape and --synthetic exclude each other")
    for name in ("shape", "synthetic"):
        v = getattr(opts, name)
        if v is not None and min(v) < 1:
            ap.error(f"--{name}: C, H and W must be >= 1")
    for name in ("height", "width", "chunk"):
        v = getattr(opts, name)
        if v is not None and v < 1:
            ap.error(f"--{name} must be >= 1")
    if opts.scale is not None and not opts.scale > 0:
        ap.error("--scale must be positive")
    if opts.compare:
        if opts.shape is not None:
            ap.error("--compare needs the data: --synthetic C,H,W or the config's scan, not --shape")
        if any(getattr(opts, k) is not None for k in ("scale", "height", "width", "window", "coils")):
            ap.error("--compare is valid on the native grid, full window, all coils only "
                     "(drop --scale / --height / --width / --window / --coils)")
    if opts.expand_coils and opts.coils is not None:
        ap.error("--expand-coils needs all virtual coils (drop --coils)")
    if opts.band_report is not None:
        if not opts.compare:
            ap.error("--band-report needs --compare (the report is the prediction's error against the data)")
    return opts


def main(argv=None) -> None:
    opts = parse_args(argv)
    from .cli import cli_fit_data, get_config
    from .coils import CoilCompression
    from .trainer_base import set_default_configs
    config = set_default_configs(get_config(opts.config))
    multiscale = config["model"] in MULTISCALE_MODELS
    image = None
    checkpoint = torch.load(opts.checkpoint, map_location="cuda")
    stored = checkpoint.get("coil_compression") if isinstance(checkpoint, dict) else None
    stored = None if stored is None else CoilCompression.from_state(stored)
    if opts.expand_coils and stored is None:
        raise SystemExit("--expand-coils: the checkpoint carries no coil compression")
    if opts.shape is not None:
        shape = tuple(opts.shape)
    else:
        # the data go through the STORED matrix (or through none): a compression is never recomputed here
        data_opts = argparse.Namespace(synthetic=None if opts.synthetic is None else ",".join(str(v) for v in opts.synthetic))
        image, _, shape, _ = cli_fit_data(data_opts, dict(config, virtual_coils=0), "max" if multiscale else "coil",
                                          image_space=bool(config.get("transform", False)) and not multiscale,
                                          matrix=stored)
    rec = Reconstructor(config, checkpoint, shape, "cuda", radii=opts.radii)
    torch.cuda.synchronize()
    t0 = time.time()
    pred = rec.render(opts.height, opts.width, opts.scale, opts.window, opts.coils, opts.chunk)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    rows = pred.numel() // 2
    res = {"shape": list(pred.shape[:3]), "rows": rows, "seconds": seconds, "rows_per_s": rows / max(seconds, 1e-12)}
    if opts.compare:
        from .bands import flag_bounds, format_band_table
        res.update(rec.compare(pred, image, bands=flag_bounds(opts.band_report)))
        if "bands" in res:
            print(format_band_table(res["bands"]), flush=True)
    if rec.coil_compression is not None:
        res["coil_compression"] = rec.coil_compression.summary()
    if rec.ring_table is not None:
        res["ring_normalization"] = rec.ring_table.summary()
    res["files"] = rec.save(opts.output_path, pred)
    if opts.expand_coils:
        res["files"].append(os.path.join(opts.output_path, "recon_physical.npy"))
        np.save(res["files"][-1], rec.expand(pred).cpu().numpy())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
