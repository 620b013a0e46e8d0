"""Mixture-of-heads fits: the reference's train_variations/train_multihead*.py and train_mix.py over its
``MultiHeadWrapper`` with ``backbone=None`` (models/networks.py:275-328) -- K expert networks on the same encoded
coordinates and a small gate network that reads the k-space radius; the prediction is the gate-weighted sum of the
experts, and every expert is also trained on its own k-means ring:

    res = clamp(sum_k w_k expert_k(gamma(coords)), -1, 1),      w = gate(z),  gate = FFN 2 -> 128 x 5 -> K (sigmoid output)
    loss = L(res, gt; sampled rows) + sum_k L(expert_k, gt; sampled rows of ring k)        (means over their own rows)

Kept from the reference: the construction and RNG order (encoder, experts 0..K-1, gate), the single Adam over experts then
gate (elementwise, so one update per engine with the same lr, betas, weight decay and per-epoch schedule is the same
update), the rings of clustering.partition_kspace with both ends included, the clamp of ``last_tanh=True``, ``detach_outs``
as ``mixture.detach``, the key names a ModuleList would give (``heads.{k}.*``, ``weighted_avg.model.N.weight|bias``).
Decided here, because none of the reference's drivers can run as written: the gate reads z [B,2] =
(coil coordinate, k-space radius), gain.gain_inputs as in the learned-gain fit; the off-ring multipliers (1e-5 / 1e-8) and
the per-ring rescaling are dropped; there is no jitter.  Experts stacked on a shared backbone are out of scope (inr_backward
gives no gradient with respect to a plan's input).  Batches, the epoch loop, validation, pictures and the band report are
ResidentFit's.

One step is tier 1 throughout: inr_forward of the K + 1 plans (stashing), inr_mix_loss_grad (csrc/inr_mix.hip: the mix, the
K + 1 loss terms and every output gradient in one pass), inr_backward of the K + 1, inr_adam_step of the K + 1.  The
per-batch row counts of the rings are taken once per epoch's rows (one batched op, one read-back) and cached per batch:
no host read inside a step.

CLI: python -m inr_mi355x.train_multihead --config C [--output_path O] [--synthetic C,H,W] [--max_steps N] [--val]
         [--save-images] [--shuffle] [--shuffle-seed S] [--band-report [N]] [--virtual-coils K]
Config: ``partition: {no_steps, no_models}`` (K = no_models, 2..8) and the optional ``mixture: {detach: true, clamp: true,
gate: {network_width, network_depth}}``.  Every validation record, metrics() and the final JSON line carry ``mixture``:
heads, detach, clamp, radii and per head the min / max / mean of the gate's weight over the whole grid (from the
validation's own sweep); a validation record also carries ``loss_terms``, the K + 1 terms of the last step.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .checkpoint import Part, joined_net, joined_optimizer_state, load_parts
from .cli import cli_fit_data, cli_fits, parse_cli, run_cli
from .engine import LossSpec
from .gain import gain_inputs
from .mix import MAX_HEADS, check_radii, inv_counts, mix_apply, mix_loss_grad
from .networks import FFN
from .train import MFN_MODELS, MODELS
from .trainer_base import ResidentFit, mlp_engine, set_default_configs

GATE_NET = {"network_input_size": 2, "network_depth": 5, "network_width": 128}  # networks.py:293-299 (+ output size K)
GATE_KEYS = ("network_width", "network_depth")
MIXTURE_KEYS = ("detach", "clamp", "gate")
HEAD_PREFIX, GATE_PREFIX = "heads.", "weighted_avg."


def mixture_settings(config: dict) -> dict:
    """{'detach', 'clamp', 'gate': {width, depth}} of config['mixture'] with the reference's defaults (detach_outs=True,
    last_tanh=True, a 128 x 5 gate)"""
    over = config.get("mixture") or {}
    unknown = sorted(set(over) - set(MIXTURE_KEYS))
    if unknown:
        raise ValueError(f"config['mixture'] takes {list(MIXTURE_KEYS)}, got {unknown}")
    gate_over = over.get("gate") or {}
    unknown = sorted(set(gate_over) - set(GATE_KEYS))
    if unknown:
        raise ValueError(f"config['mixture']['gate'] takes {list(GATE_KEYS)}, got {unknown}")
    gate = {k: int(gate_over.get(k, GATE_NET[k])) for k in GATE_KEYS}
    if gate["network_depth"] < 2 or gate["network_width"] < 1:
        raise ValueError(f"config['mixture']['gate'] = {gate_over!r}: depth >= 2 and width >= 1")
    return {"detach": bool(over.get("detach", True)), "clamp": bool(over.get("clamp", True)), "gate": gate}


def gate_net(settings: dict, K: int) -> dict:
    """the gate's FFN parameters: 2 -> width x depth -> K"""
    return dict(GATE_NET, network_output_size=int(K), **settings["gate"])


def has_head_keys(net_state: dict) -> bool:
    return any(k.startswith(HEAD_PREFIX) for k in net_state)


def merge_state(experts: Sequence[dict], gate: dict) -> OrderedDict:
    """MultiHeadWrapper.state_dict() with its heads in a ModuleList: 'heads.{k}.' + expert k's keys, then 'weighted_avg.'
    + the gate FFN's (clones: a checkpoint must not alias the running weights).  Kept for callers outside the package:
    the trainer writes the same keys through checkpoint.joined_net over its _parts()."""
    net = OrderedDict()
    for prefix, sd in [(f"{HEAD_PREFIX}{k}.", sd) for k, sd in enumerate(experts)] + [(GATE_PREFIX, gate)]:
        net.update((prefix + name, v.detach().clone()) for name, v in sd.items())
    return net


def split_state(net_state: dict):
    """([expert state_dicts in head order], gate state_dict) of merge_state's"""
    experts, gate = {}, OrderedDict()
    for name, v in net_state.items():
        if name.startswith(GATE_PREFIX):
            gate[name[len(GATE_PREFIX):]] = v
        elif name.startswith(HEAD_PREFIX):
            k, _, rest = name[len(HEAD_PREFIX):].partition(".")
            if not k.isdigit() or not rest:
                raise ValueError(f"key {name!r}: expected 'heads.<k>.<parameter>'")
            experts.setdefault(int(k), OrderedDict())[rest] = v
        else:
            raise ValueError(f"key {name!r} outside 'heads.' / 'weighted_avg.'")
    if sorted(experts) != list(range(len(experts))) or not experts or not gate:
        raise ValueError(f"heads {sorted(experts)} and {len(gate)} gate keys: expected heads 0..K-1 and a gate")
    return [experts[k] for k in range(len(experts))], gate


def wrong_checkpoint(net_state: dict) -> str:
    """which module loads a checkpoint that is no mixture's"""
    if any(k.startswith("scaler.") for k in net_state):
        return ("the checkpoint has 'scaler.' keys and no 'heads.' keys: it is a learned-gain fit's -- load it with "
                "ScaledFitTrainer (python -m inr_mi355x.train_scaling)")
    return ("the checkpoint has no 'heads.' keys: it is a plain fit's -- load it with INRTrainer "
            "(python -m inr_mi355x.train)")


def mixture_heads(config: dict, radii: Optional[Sequence[float]] = None) -> int:
    if radii is not None:
        return len(radii) - 1
    part = config.get("partition") or {}
    if "no_models" not in part:
        raise ValueError("a mixture-of-heads fit needs config['partition'] = {no_steps, no_models} (or radii=)")
    return int(part["no_models"])


def check_mixture_config(config: dict, world: int = 1, graph_steps: bool = False,
                         radii: Optional[Sequence[float]] = None) -> None:
    """What a mixture-of-heads fit cannot be combined with -- refused before anything is allocated."""
    name = config["model"]
    if name in MFN_MODELS:
        raise NotImplementedError(f"model {name!r}: mixture-of-heads fits mix SIREN / FFN / WIRE / WIRE2D experts "
                                  "(MultiHeadWrapper's heads), not the filter networks")
    if name not in MODELS:
        raise NotImplementedError(f"model {name!r} has no MI355X kernel yet (have {sorted(set(MODELS) - set(MFN_MODELS))})")
    if config.get("optimizer", "Adam") != "Adam":
        raise NotImplementedError("only Adam (train_multihead.py:84-87)")
    if config.get("precision", "f32") != "f32":
        raise NotImplementedError(f"precision {config['precision']!r}: mixture-of-heads fits run the fp32 tier-1 calls")
    if config["per_coil"] or config["use_tv"]:
        raise NotImplementedError("per_coil / use_tv: mixture-of-heads fits train on plain batches")
    if config.get("loss") == "LSL":
        raise NotImplementedError("loss 'LSL' (CenterLoss): its random-pair term is not part of inr_mix_loss_grad")
    if config.get("loss") == "FFL":
        raise NotImplementedError("loss 'FFL' (focal frequency loss): inr_mix_loss_grad forms its terms through loss_row; "
                                  "FFL fits run in INRTrainer (python -m inr_mi355x.train) only")
    if config["regularization"]["type"] != "none":
        raise NotImplementedError(f"regularization {config['regularization']['type']!r}: the penalty is over all "
                                  "parameters of every network and would couple the engines")
    if config["trajectory"] not in (None, "none"):
        raise NotImplementedError(f"config['trajectory'] = {config['trajectory']!r}: off-grid fits run in INRTrainer "
                                  "(python -m inr_mi355x.train) only")
    if config.get("ring_normalization") not in (None, "none", False):
        raise NotImplementedError(f"config['ring_normalization'] = {config['ring_normalization']!r}: the reference's "
                                  "per-ring rescaling is not part of the mixture; ring-normalised fits run in INRTrainer "
                                  "(python -m inr_mi355x.train) only")
    if config.get("row_sampling") not in (None, "none", False):
        raise NotImplementedError(f"config['row_sampling'] = {config['row_sampling']!r}: weighted epochs run in INRTrainer "
                                  "(python -m inr_mi355x.train) only")
    if graph_steps:
        raise NotImplementedError("graph_steps: a mixture-of-heads step is a sequence of tier-1 calls on K + 1 plans")
    if world > 1:
        raise NotImplementedError("mixture-of-heads fits run on one rank")
    K = mixture_heads(config, radii)
    if K < 2 or K > MAX_HEADS:
        raise NotImplementedError(f"{K} heads: a mixture has 2..{MAX_HEADS} (config['partition']['no_models'])")
    if int(config["net"].get("network_output_size", 2)) != 2:
        raise NotImplementedError(f"network_output_size = {config['net']['network_output_size']}: the experts give "
                                  "(re, im) rows")
    mixture_settings(config)


class MixtureFitTrainer(ResidentFit):
    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, shape, device, seed: int = 0,
                 mask: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1, process_group=None,
                 mask_seed: Optional[int] = None, graph_steps: bool = False, coil_compression=None,
                 radii: Optional[Sequence[float]] = None):
        check_mixture_config(set_default_configs(dict(config)), world, graph_steps, radii)
        self.mixture = mixture_settings(config)
        config = self._init_fit(config, shape, device, seed, rank, world, process_group, False, coil_compression)
        self.in_image_space = bool(config.get("transform", False))
        C, H, W = int(shape[0]), int(shape[1]), int(shape[2])
        if radii is None:  # before the seed, as in the ring ensemble (train_multihead.py:102-107)
            from .clustering import partition_kspace
            part = config["partition"]
            _, radii = partition_kspace(image.to(self.device).reshape(C, H, W, 2),
                                        coords.to(self.device).reshape(C, H, W, 3),
                                        no_steps=part["no_steps"], no_parts=part["no_models"])
        # the edges as fp32 numbers: the kernel, the counts below and the float64 statement compare the same values
        self.radii = check_radii([float(np.float32(r)) for r in radii], len(radii) - 1)
        self.K = len(self.radii) - 1
        self.gate_params = gate_net(self.mixture, self.K)
        # encoder, experts 0..K-1, gate on one CPU generator
        self._seeded_encoder(seed)
        self.models, made = [], []
        for _ in range(self.K):
            self.models.append(MODELS[config["model"]](config["net"]))
        self.gate = FFN(self.gate_params)
        for k in range(self.K):
            m = self.models[k] = self.models[k].to(self.device)
            made.append(mlp_engine(m, self.encoder, config["encoder"]))
        self.engines, self.enc_B = [eng for eng, _ in made], made[0][1]  # one encoder: every expert got the same matrix
        self.gate = self.gate.to(self.device)
        self.gate_engine = self.gate._engine()  # an INR_INPUT_X plan on z
        self.model, self.engine = self.models[0], self.engines[0]  # ResidentFit's test loss runs inr_loss_grad through it
        self.loss = LossSpec.from_config(config)
        self._resident_data(image, coords, config["undersampling"], mask, mask_seed, False)
        self.z = self._t_z = gain_inputs(self.coords)
        self.dist = self._t_dist = self.z[:, 1].contiguous()
        self._mix_loss = torch.zeros(L.LOSS_WORDS, device=self.device)
        self._inv = self._batch_inv_counts(self._t_dist, self._t_mask if self.mask is not None else None) \
            if self._epoch_buf is None else []
        self._gate_parts = None
        self._last_gate = None
        self._finish_init()

    # ---- per-batch counts ------------------------------------------------------------------------
    def _batch_inv_counts(self, dist: torch.Tensor, mask: Optional[torch.Tensor]) -> List[List[float]]:
        """[1/count_0 .. 1/count_K] of every training batch of these rows: one batched op, one read-back"""
        live = torch.ones_like(dist, dtype=torch.bool) if mask is None else mask != 0
        flags = torch.stack([live] + [live & (dist >= self.radii[k]) & (dist <= self.radii[k + 1])
                                      for k in range(self.K)])
        cum = torch.cumsum(flags.to(torch.int64), dim=-1)
        n = int(dist.shape[0])
        ends = torch.arange(1, self.steps_per_epoch + 1, device=dist.device).mul_(self.bs).clamp_(max=n) - 1
        at = cum.index_select(-1, ends)
        counts = torch.diff(at, dim=-1, prepend=torch.zeros_like(at[..., :1])).t().tolist()
        return [inv_counts(c) for c in counts]

    def _refilled(self) -> None:
        """The epoch buffers hold a new epoch's rows: z and the radius from the epoch's coordinates, every batch's ring
        counts, and the HDR scalar of every batch."""
        self._t_z = gain_inputs(self._t_coords)
        self._t_dist = self._t_z[:, 1].contiguous()
        self._inv = self._batch_inv_counts(self._t_dist, self._t_mask if self.mask is not None else None)
        self._refill_hdr_A()

    # ---- one optimizer step ----------------------------------------------------------------------
    def _parts(self):
        """experts in head order (the encoder travels with expert 0), then the gate"""
        experts = [Part(f"{HEAD_PREFIX}{k}.", m, eng) for k, (m, eng) in enumerate(zip(self.models, self.engines))]
        experts[0] = experts[0]._replace(encoder=self.encoder, rebind=self._rebind_encoder)
        return experts + [Part(GATE_PREFIX, self.gate, self.gate_engine)]

    def step(self, epoch: int, it: int) -> torch.Tensor:
        if self.shuffle:
            it = self._begin_shuffled(epoch, it)
        lo, hi = self._range(it)
        A = self._hdr_A_epoch[it] if self._epoch_buf is not None and self._hdr_A_epoch else self._batch_hdr_A(it, lo, hi)
        cfg, lr = self.config, self._lr(epoch)
        x, z, gt = self._inputs(lo, hi, True), self._t_z[lo:hi], self._t_image[lo:hi]
        m = self._t_mask[lo:hi] if self.mask is not None else None
        ys = [eng.forward(x, self.enc_B, save=True) for eng in self.engines]
        w = self.gate_engine.forward(z, None, save=True)
        out, _, dys, dw = mix_loss_grad(self.loss, ys, w, gt, self._t_dist[lo:hi], self.radii, self._inv[it], mask=m,
                                        detach=self.mixture["detach"], clamp=self.mixture["clamp"], hdr_A=A,
                                        want_res=False, loss_out=self._mix_loss)
        for eng, dy in zip(self.engines, dys):
            eng.backward(x, self.enc_B, dy)
        self.gate_engine.backward(z, None, dw)
        for part in self._parts():
            part.engine.adam_step(lr, cfg["beta1"], cfg["beta2"], 1e-8, cfg["weight_decay"])
        self.global_step += 1
        return out[0]

    def loss_terms(self) -> List[float]:
        """[mixed term, ring 0 .. ring K-1] of the last step (one host read)"""
        return self._mix_loss[1:self.K + 2].tolist()

    # ---- validation ------------------------------------------------------------------------------
    def _forward_chunk(self, lo: int, hi: int) -> torch.Tensor:
        x = self._inputs(lo, hi)
        ys = [eng.forward(x, self.enc_B, save=False) for eng in self.engines]
        w = self.gate_engine.forward(self.z[lo:hi], None, save=False)
        if self._gate_parts is not None:
            wd = w.double()
            self._gate_parts.append(torch.stack((wd.min(0).values, wd.max(0).values, wd.sum(0))))
        return mix_apply(ys, w, clamp=self.mixture["clamp"], out=ys[0])

    @torch.no_grad()
    def _predict_raw(self, chunk: Optional[int] = None) -> torch.Tensor:
        """the sweep, and from its own forward the gate's weights over the whole grid (one host read)"""
        self._gate_parts = []
        try:
            pred = super()._predict_raw(chunk)
            parts = torch.stack(self._gate_parts).cpu()  # [chunks, 3, K]
        finally:
            self._gate_parts = None
        self._last_gate = {"min": parts[:, 0].min(0).values.tolist(), "max": parts[:, 1].max(0).values.tolist(),
                           "mean": (parts[:, 2].sum(0) / self.n).tolist()}
        return pred

    @property
    def mixture_summary(self) -> Optional[dict]:
        """{'heads', 'detach', 'clamp', 'radii', 'gate': {'min', 'max', 'mean'} per head, 'gate_width', 'gate_depth'} --
        'gate' from the last sweep (None before the first)"""
        return {"heads": self.K, "detach": self.mixture["detach"], "clamp": self.mixture["clamp"],
                "radii": list(self.radii), "gate": self._last_gate,
                "gate_width": self.gate_params["network_width"], "gate_depth": self.gate_params["network_depth"]}

    @torch.no_grad()
    def validate(self, epoch: int) -> dict:
        terms = self.loss_terms() if self.global_step else None  # before the test loss reuses any loss buffer
        rec = self._validated(epoch, self._predict_raw())
        rec["mixture"] = self.mixture_summary
        rec["loss_terms"] = terms
        return rec

    @torch.no_grad()
    def metrics(self) -> dict:
        rec = super().metrics()
        rec["mixture"] = self.mixture_summary
        return rec

    # ---- checkpoints -----------------------------------------------------------------------------
    def checkpoint(self) -> dict:
        """{'net', 'enc', 'opt', 'mixture'}: 'net' with the key names of a MultiHeadWrapper whose heads sit in a ModuleList,
        'opt' in torch.optim.Adam.state_dict() layout over the experts' parameters in head order, then the gate's."""
        parts = self._parts()
        ckpt = {"net": joined_net(parts), "enc": None if self.encoder.B is None else self.encoder.B.clone(),
                "opt": joined_optimizer_state(parts, self.config),
                "mixture": {"radii": list(self.radii), "detach": self.mixture["detach"], "clamp": self.mixture["clamp"]}}
        if self.coil_compression is not None:
            ckpt["coil_compression"] = self.coil_compression.state()
        return ckpt

    def load_checkpoint(self, ckpt: dict) -> None:
        if not has_head_keys(ckpt["net"]):
            raise ValueError(wrong_checkpoint(ckpt["net"]))
        self._check_same_compression(ckpt)
        experts, gate = split_state(ckpt["net"])
        if len(experts) != self.K:
            raise ValueError(f"the checkpoint has {len(experts)} heads, the trainer {self.K}")
        mix = ckpt.get("mixture")
        if mix is not None and [float(np.float32(r)) for r in mix["radii"]] != self.radii:
            raise ValueError(f"checkpoint and trainer disagree: radii {mix['radii']} against {self.radii}")
        load_parts(self._parts(), experts + [gate], [ckpt.get("enc")] + [None] * self.K, ckpt.get("opt"))


def main():
    opts, config = parse_cli()
    for cfg, fit_opts in cli_fits(config, opts):
        image, coords, shape, cc = cli_fit_data(opts, cfg, "coil", image_space=bool(cfg.get("transform", False)))
        run_cli(MixtureFitTrainer(cfg, image, coords, shape, "cuda", coil_compression=cc), cfg, fit_opts)


if __name__ == "__main__":
    main()
