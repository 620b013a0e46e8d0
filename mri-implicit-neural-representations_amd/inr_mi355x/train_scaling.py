"""Learned radial gain fits: the reference's train_variations/train_scaling.py over its ``ScalerWrapper``
(models/networks.py:380-405) -- a backbone and a second small network that learns, together with the fit, the radial
gain the k-space magnitude falls by:

    res = backbone(gamma(coords)) * exp(-scaler(z)),        scaler = FFN 2 -> 512 x 8 -> 1 (sigmoid output)

Kept from the reference: the construction and RNG order (encoder, backbone, gain network), the single Adam over both
networks' parameters (elementwise, so one update per engine with the same lr, betas, weight decay and per-epoch schedule
is the same update), the loss on ``res``, the checkpoint's key names (``backbone.*``, ``scaler.model.N.weight|bias``).
Decided here, because the reference script cannot run (it hands ``dist_to_center`` [B] to a Linear(2, 512)): the gain
network reads z [B,2] = (coil coordinate, k-space radius), the only two-column companion the reference's dataset offers
(INTEGRATION.md section 4).  Batches, the epoch loop, validation, pictures and the band report are ResidentFit's.

One step is tier 1 throughout: inr_forward of both plans (stashing), inr_gain_loss_grad (csrc/inr_gain.hip: the product,
the loss and both output gradients in one pass), inr_backward of both, inr_adam_step of both.

CLI: python -m inr_mi355x.train_scaling --config C [--output_path O] [--synthetic C,H,W] [--max_steps N] [--val]
         [--save-images] [--shuffle] [--shuffle-seed S] [--band-report [N]] [--virtual-coils K]
The optional config key ``scaler: {network_width, network_depth}`` sizes the gain network (default 512 x 8, the
reference's).  Every validation record, metrics() and the final JSON line carry ``gain``: min / max / mean of exp(-s)
over the whole grid (from the validation's own sweep) and the gain network's width and depth.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from .checkpoint import Part, joined_net, joined_optimizer_state, load_parts, split_prefixed
from .cli import cli_fit_data, cli_fits, parse_cli, run_cli
from .engine import LossSpec
from .gain import gain_apply, gain_inputs, gain_loss_grad
from .networks import FFN
from .train import MFN_MODELS, MODELS
from .trainer_base import ResidentFit, mlp_engine, set_default_configs

SCALER_NET = {"network_input_size": 2, "network_output_size": 1, "network_depth": 8, "network_width": 512}  # networks.py:388-393
SCALER_KEYS = ("network_width", "network_depth")
PREFIXES = ("backbone.", "scaler.")


def scaler_net(config: dict) -> dict:
    """the gain network's FFN parameters: the reference's, with config['scaler'] overriding width and depth"""
    net = dict(SCALER_NET)
    over = config.get("scaler") or {}
    unknown = sorted(set(over) - set(SCALER_KEYS))
    if unknown:
        raise ValueError(f"config['scaler'] takes {list(SCALER_KEYS)}, got {unknown}")
    for k in SCALER_KEYS:
        if k in over:
            net[k] = int(over[k])
    if net["network_depth"] < 2 or net["network_width"] < 1:
        raise ValueError(f"config['scaler'] = {over!r}: depth >= 2 and width >= 1")
    return net


def has_scaler_keys(net_state: dict) -> bool:
    return any(k.startswith("scaler.") for k in net_state)


def wrapper_state(backbone, scaler) -> OrderedDict:
    """ScalerWrapper.state_dict() of the two models: 'backbone.' + the backbone's keys, then 'scaler.' + the FFN's
    (clones: a checkpoint must not alias the running weights)"""
    return joined_net([Part(p, m, None) for p, m in zip(PREFIXES, (backbone, scaler))])


def split_state(net_state: dict):
    """(backbone state_dict, gain-network state_dict) of a ScalerWrapper's"""
    return tuple(split_prefixed(net_state, PREFIXES))


def check_scaled_config(config: dict, world: int = 1, graph_steps: bool = False) -> None:
    """What a learned-gain fit cannot be combined with -- refused before anything is allocated."""
    name = config["model"]
    if name in MFN_MODELS:
        raise NotImplementedError(f"model {name!r}: learned-gain fits wrap SIREN / FFN / WIRE / WIRE2D (ScalerWrapper's "
                                  "backbones), not the filter networks")
    if name not in MODELS:
        raise NotImplementedError(f"model {name!r} has no MI355X kernel yet (have {sorted(set(MODELS) - set(MFN_MODELS))})")
    if config.get("optimizer", "Adam") != "Adam":
        raise NotImplementedError("only Adam (train_scaling.py:69-72)")
    if config.get("precision", "f32") != "f32":
        raise NotImplementedError(f"precision {config['precision']!r}: learned-gain fits run the fp32 tier-1 calls")
    if config["per_coil"] or config["use_tv"]:
        raise NotImplementedError("per_coil / use_tv: learned-gain fits train on plain batches")
    if config.get("loss") == "LSL":
        raise NotImplementedError("loss 'LSL' (CenterLoss): its random-pair term is not part of inr_gain_loss_grad")
    if config.get("loss") == "FFL":
        raise NotImplementedError("loss 'FFL' (focal frequency loss): inr_gain_loss_grad forms its loss through loss_row; "
                                  "FFL fits run in INRTrainer (python -m inr_mi355x.train) only")
    if config["regularization"]["type"] != "none":
        raise NotImplementedError(f"regularization {config['regularization']['type']!r}: the penalty is over all "
                                  "parameters of both networks and would couple the two engines")
    if config["trajectory"] not in (None, "none"):
        raise NotImplementedError(f"config['trajectory'] = {config['trajectory']!r}: off-grid fits run in INRTrainer "
                                  "(python -m inr_mi355x.train) only")
    if config.get("ring_normalization") not in (None, "none", False):
        raise NotImplementedError(f"config['ring_normalization'] = {config['ring_normalization']!r}: the gain is learned "
                                  "here; ring-normalised fits run in INRTrainer (python -m inr_mi355x.train) only")
    if config.get("row_sampling") not in (None, "none", False):
        raise NotImplementedError(f"config['row_sampling'] = {config['row_sampling']!r}: weighted epochs run in INRTrainer "
                                  "(python -m inr_mi355x.train) only")
    if graph_steps:
        raise NotImplementedError("graph_steps: a learned-gain step is a sequence of tier-1 calls on two plans")
    if world > 1:
        raise NotImplementedError("learned-gain fits run on one rank")


class ScaledFitTrainer(ResidentFit):
    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, shape, device, seed: int = 0,
                 mask: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1, process_group=None,
                 mask_seed: Optional[int] = None, graph_steps: bool = False, coil_compression=None):
        check_scaled_config(set_default_configs(dict(config)), world, graph_steps)
        self.scaler_params = scaler_net(config)
        config = self._init_fit(config, shape, device, seed, rank, world, process_group, False, coil_compression)
        self.in_image_space = bool(config.get("transform", False))
        # encoder, backbone, gain network on one CPU generator (train_scaling.py:46-66); the backbone moves to the device
        # before the wrapper builds its FFN, which draws nothing
        self._seeded_encoder(seed)
        self.model = MODELS[config["model"]](config["net"]).to(self.device)
        self.scaler = FFN(self.scaler_params).to(self.device)
        self.engine, self.enc_B = mlp_engine(self.model, self.encoder, config["encoder"])
        self.scaler_engine = self.scaler._engine()  # an INR_INPUT_X plan on z
        self.loss = LossSpec.from_config(config)
        self._resident_data(image, coords, config["undersampling"], mask, mask_seed, False)
        self.z = self._t_z = gain_inputs(self.coords)
        self._gain_parts = None
        self._last_gain = None
        self._finish_init()

    # ---- one optimizer step ----------------------------------------------------------------------
    def _parts(self):
        return [Part(PREFIXES[0], self.model, self.engine, self.encoder, self._rebind_encoder),
                Part(PREFIXES[1], self.scaler, self.scaler_engine)]

    def _refilled(self) -> None:
        """The epoch buffers hold a new epoch's rows: z from the epoch's coordinates (as the ring ensemble's dist), and
        the HDR scalar of every batch."""
        self._t_z = gain_inputs(self._t_coords)
        self._refill_hdr_A()

    def step(self, epoch: int, it: int) -> torch.Tensor:
        if self.shuffle:
            it = self._begin_shuffled(epoch, it)
        lo, hi = self._range(it)
        count = self._count(lo, hi)
        A = self._hdr_A_epoch[it] if self._epoch_buf is not None and self._hdr_A_epoch else self._batch_hdr_A(it, lo, hi)
        cfg, lr = self.config, self._lr(epoch)
        x, z, gt = self._inputs(lo, hi, True), self._t_z[lo:hi], self._t_image[lo:hi]
        m = self._t_mask[lo:hi] if self.mask is not None else None
        yb = self.engine.forward(x, self.enc_B, save=True)
        sb = self.scaler_engine.forward(z, None, save=True)
        loss, _, dy, ds = gain_loss_grad(self.loss, yb, sb.view(-1), gt, count, mask=m, hdr_A=A, want_res=False,
                                         loss_out=self.engine._loss)
        self.engine.backward(x, self.enc_B, dy)
        self.scaler_engine.backward(z, None, ds.view(-1, 1))
        for part in self._parts():
            part.engine.adam_step(lr, cfg["beta1"], cfg["beta2"], 1e-8, cfg["weight_decay"])
        self.global_step += 1
        return loss

    # ---- validation ------------------------------------------------------------------------------
    def _forward_chunk(self, lo: int, hi: int) -> torch.Tensor:
        y = self.engine.forward(self._inputs(lo, hi), self.enc_B, save=False)
        s = self.scaler_engine.forward(self.z[lo:hi], None, save=False).view(-1)
        if self._gain_parts is not None:
            g = torch.exp(-s.double())
            self._gain_parts.append(torch.stack((g.min(), g.max(), g.sum())))
        return gain_apply(y, s, out=y)

    @torch.no_grad()
    def _predict_raw(self, chunk: Optional[int] = None) -> torch.Tensor:
        """the sweep, and from its own forward the gain exp(-s) over the whole grid (one host read)"""
        self._gain_parts = []
        try:
            pred = super()._predict_raw(chunk)
            parts = torch.stack(self._gain_parts).cpu()
        finally:
            self._gain_parts = None
        self._last_gain = {"min": float(parts[:, 0].min()), "max": float(parts[:, 1].max()),
                           "mean": float(parts[:, 2].sum()) / self.n, "width": self.scaler_params["network_width"],
                           "depth": self.scaler_params["network_depth"]}
        return pred

    @property
    def gain_summary(self) -> Optional[dict]:
        """{'min', 'max', 'mean', 'width', 'depth'} of the last sweep (None before the first)"""
        return self._last_gain

    @torch.no_grad()
    def validate(self, epoch: int) -> dict:
        rec = self._validated(epoch, self._predict_raw())
        rec["gain"] = self._last_gain
        return rec

    @torch.no_grad()
    def metrics(self) -> dict:
        rec = super().metrics()
        rec["gain"] = self._last_gain
        return rec

    # ---- checkpoints -----------------------------------------------------------------------------
    def checkpoint(self) -> dict:
        """{'net', 'enc', 'opt'} as train_scaling.py:220-223 writes it: 'net' with ScalerWrapper's state_dict keys, 'opt'
        in torch.optim.Adam.state_dict() layout over model.parameters() -- the backbone's parameters, then the gain
        network's."""
        parts = self._parts()
        ckpt = {"net": joined_net(parts), "enc": None if self.encoder.B is None else self.encoder.B.clone(),
                "opt": joined_optimizer_state(parts, self.config)}
        if self.coil_compression is not None:
            ckpt["coil_compression"] = self.coil_compression.state()
        return ckpt

    def load_checkpoint(self, ckpt: dict) -> None:
        if not has_scaler_keys(ckpt["net"]):
            raise ValueError("the checkpoint has no 'scaler.' keys: it is a plain fit's -- load it with INRTrainer "
                             "(python -m inr_mi355x.train)")
        self._check_same_compression(ckpt)
        load_parts(self._parts(), split_state(ckpt["net"]), [ckpt.get("enc"), None], ckpt.get("opt"))


def main():
    opts, config = parse_cli()
    for cfg, fit_opts in cli_fits(config, opts):
        image, coords, shape, cc = cli_fit_data(opts, cfg, "coil", image_space=bool(cfg.get("transform", False)))
        run_cli(ScaledFitTrainer(cfg, image, coords, shape, "cuda", coil_compression=cc), cfg, fit_opts)


if __name__ == "__main__":
    main()
