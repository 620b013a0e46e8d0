"""SENSE-model fits (no reference counterpart): every other fit here treats the C coils of a scan
as C unrelated pictures.  This one has the physics that makes undersampled reconstruction work -- all coils show the same
anatomy through different smooth sensitivity maps -- as two coordinate networks in IMAGE space, fitted to K-SPACE data:

    I(y, x)      the image network, MODELS[config['model']](config['net']) with 2 outputs (one complex number); its
                 input is the dataset's coordinate row with the coil column set to 0
    S(c, y, x)   the sensitivity network, an FFN (64 x 4 unless config['sense']['net'] says otherwise) with 2 outputs on
                 the dataset's coordinate row as it is, behind an encoder of its own (scale 1.0: coil maps are smooth)
    X_g = scale * S_g * I,   K_g = fft2c(X_g),   loss = the config's pointwise loss on (K, gt, mask)

One step takes one group of up to G = coils_per_step consecutive coils (the last group is smaller when G does not divide
C) and is tier 1 throughout: inr_forward of both plans (stashing H*W and G*H*W rows), inr_sense_apply(shift = 1),
torch.fft.fft2(ortho), inr_loss_grad, torch.fft.ifft2(ortho), inr_sense_grad, inr_backward of both, inr_adam_step of
both with the same lr, betas, weight decay and per-epoch schedule.  No shifted copy is made in a step: targets and mask
are stored ifftshift-ed once at ingest (per coil, over H x W), the product kernel writes every pixel where ifftshift
would put it, and every loss kind of inr_loss_grad is independent of row order.  fftshift is applied only where a
prediction leaves the trainer (predict_all and what is built on it: validation, pictures, the band report).

Config key ``sense`` (all optional): coils_per_step (default: all coils), scale (default: the RMS of the zero-filled coil
images, so that O(1) network outputs start at the data's magnitude), net {network_width, network_depth}, encoder {scale,
embedding_size}, max_stash_bytes (default 8 GB: the sensitivity plan's activation stash for G*H*W rows must fit, or the
trainer refuses with the largest coils_per_step that does).  Every undersampling pattern and an explicit mask work.

CLI: python -m inr_mi355x.train_sense --config C [--output_path O] [--synthetic C,H,W] [--max_steps N] [--val]
         [--save-images] [--shuffle] [--shuffle-seed S] [--band-report [N]]
Every validation record, metrics() and the final JSON line carry ``sense``: coils_per_step, scale, the sensitivity
network's width and depth, and min / max / mean over the grid of sens_rss = sqrt(sum_c |S_c|^2).

``sense.maps: calibrated`` (--sense-maps calibrated): the sensitivities are not learned but
estimated ONCE from the fully sampled centre of k-space (sense_calib.py: ``sense.calib`` {size [a, b], window, floor, acs};
with ``acs`` the block is OR-ed into every coil's sampling mask first) and stay fixed.  The sensitivity network, its stash,
its backward and its Adam update are gone; a step takes every coil and needs the image half of the adjoint alone
(inr_sense_adjoint).  ``sense.baseline: cg-N`` (--sense-baseline) adds CG-SENSE from the same maps and samples, scored as
the fit is, to every record as ``cg_sense``.

``sense.prior: {kind: tv, weight, eps}`` (--sense-prior tv:WEIGHT[:EPS]), with either maps mode:
smoothed isotropic total variation of the image network's output I (not of scale * I) is added to every step's loss.
After inr_sense_adjoint / inr_sense_grad has written dimg, inr_image_tv_grad adds weight * dTV/dI into it; the step
returns data loss + weight * TV.  With learned maps and several coil groups per epoch every group's step carries the
prior with its full weight.  Records and metrics() gain a top-level ``prior`` {kind, weight, eps, value} (the value on
the image of the prediction sweep); the validation's test loss stays data-only.  ``use_tv`` stays refused: it is the
reference's TV of a coil's predicted k-space.  With the key absent nothing changes.

``trajectory`` with ``sense.maps: calibrated`` (--trajectory, --trajectory-operator,
--trajectory-density): the fit runs on off-grid samples.  The targets are the exact NUDFT samples [C, M, 2] of the scan;
the maps are calibrated from those samples alone (density-weighted exact adjoint -> fft2c -> the usual block); a step is
forward -> sense_nufft -> inr_loss_grad -> sense_nufft_adjoint -> prior -> backward -> Adam on all coils
(sense_nufft.py).  ``trajectory_operator`` defaults to "gridding" HERE; "exact" runs the step from inr_sense_apply ->
inr_nudft and inr_adjoint_nudft -> inr_sense_adjoint.  ``sense.baseline: cg-N`` is then non-Cartesian CG-SENSE.  Learned
maps refuse a trajectory; with one, ``undersampling``, a mask, ``calib.acs``, ``trajectory_baseline`` and loss 'HDR'
are refused.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .checkpoint import Part, joined_net, joined_optimizer_state, load_parts
from .cli import cli_fit_data, cli_fits, parse_cli, run_cli
from .engine import LossSpec
from .networks import FFN, Positional_Encoder
from .sense import (IMAGE_PREFIX, SENS_PREFIX, has_sense_keys, join_state, sens_encoder_config, sense_apply,  # noqa: F401
                    sense_grad, shift_index, split_state)
from .shuffle import CoilOrder
from .train import MFN_MODELS, MODELS
from .trainer_base import ResidentFit, _encoded, mlp_engine, set_default_configs

SENSE_KEYS = ("coils_per_step", "scale", "net", "encoder", "max_stash_bytes")
MAPS_KEYS = ("maps", "calib", "baseline", "cg_lambda")  # DESIGN.md 4.29; the last three with maps: calibrated only
MAPS_MODES = ("learned", "calibrated")
PRIOR_KEYS = ("prior",)  # DESIGN.md 4.30; with either maps mode
SENS_NET = {"network_width": 64, "network_depth": 4}
SENS_NET_KEYS = ("network_width", "network_depth")
SENS_ENC_KEYS = ("scale", "embedding_size")
MAX_STASH_BYTES = 8 * 10 ** 9


def _only(over, allowed, where: str) -> dict:
    over = over or {}
    if not isinstance(over, dict):
        raise ValueError(f"{where} is a mapping of {list(allowed)}, got {over!r}")
    unknown = sorted(set(over) - set(allowed))
    if unknown:
        raise ValueError(f"{where} takes {list(allowed)}, got {unknown}")
    return over


def sense_settings(config: dict, n_coils: Optional[int] = None) -> dict:
    """config['sense'] with its defaults: {'coils_per_step' (None: all coils; clipped to ``n_coils`` when given), 'scale'
    (None: from the data), 'net' {network_width, network_depth}, 'encoder' {scale, embedding_size},
    'max_stash_bytes'}.  Unknown keys, here or under 'net' / 'encoder', raise ValueError."""
    over = _only(config.get("sense"), SENSE_KEYS + MAPS_KEYS + PRIOR_KEYS, "config['sense']")
    maps_settings(config)  # what the two modes refuse of each other
    net = dict(SENS_NET)
    net.update({k: int(v) for k, v in _only(over.get("net"), SENS_NET_KEYS, "config['sense']['net']").items()})
    if net["network_depth"] < 2 or net["network_width"] < 1:
        raise ValueError(f"config['sense']['net'] = {over.get('net')!r}: depth >= 2 and width >= 1")
    main = config.get("encoder") or {}
    enc = {"scale": 1.0, "embedding_size": main.get("embedding_size")}
    enc.update(_only(over.get("encoder"), SENS_ENC_KEYS, "config['sense']['encoder']"))
    enc["scale"] = float(enc["scale"])
    if enc["embedding_size"] is not None:
        enc["embedding_size"] = int(enc["embedding_size"])
        if enc["embedding_size"] < 1:
            raise ValueError(f"config['sense']['encoder']['embedding_size'] = {enc['embedding_size']}")
    G = over.get("coils_per_step")
    if G is not None:
        G = int(G)
        if G < 1:
            raise ValueError(f"config['sense']['coils_per_step'] = {G} (at least 1)")
        if n_coils is not None:
            G = min(G, int(n_coils))
    elif n_coils is not None:
        G = int(n_coils)
    scale = over.get("scale")
    if scale is not None:
        scale = float(scale)
        if not math.isfinite(scale) or scale == 0.0:
            raise ValueError(f"config['sense']['scale'] = {scale} (finite and not zero)")
    stash = int(over.get("max_stash_bytes", MAX_STASH_BYTES))
    if stash < 1:
        raise ValueError(f"config['sense']['max_stash_bytes'] = {stash}")
    return {"coils_per_step": G, "scale": scale, "net": net, "encoder": enc, "max_stash_bytes": stash}


def maps_settings(config: dict, H: Optional[int] = None, W: Optional[int] = None) -> Optional[dict]:
    """None for learned maps (the default: config['sense'] without 'maps', or maps: learned -- then 'calib', 'baseline'
    and 'cg_lambda' are refused), else {'maps': 'calibrated', 'calib': sense_calib.parse_calib's dict, 'baseline': N of
    cg-N or None, 'cg_lambda'} -- then 'net', 'encoder' and 'max_stash_bytes' are refused: there is no sensitivity plan.
    ValueError for every refusal."""
    from .sense_calib import parse_calib, parse_sense_baseline
    over = _only(config.get("sense"), SENSE_KEYS + MAPS_KEYS + PRIOR_KEYS, "config['sense']")
    mode = over.get("maps", "learned")
    if mode not in MAPS_MODES:
        raise ValueError(f"config['sense']['maps'] = {mode!r}: one of {list(MAPS_MODES)}")
    if mode == "learned":
        given = [k for k in MAPS_KEYS[1:] if k in over]
        if given:
            raise ValueError(f"config['sense'] has {given} but maps: learned -- they belong to maps: calibrated")
        return None
    given = [k for k in ("net", "encoder", "max_stash_bytes") if k in over]
    if given:
        raise ValueError(f"config['sense'] has {given} but maps: calibrated -- there is no sensitivity network to size")
    lam = float(over.get("cg_lambda", 0.0))
    if not math.isfinite(lam) or lam < 0.0:
        raise ValueError(f"config['sense']['cg_lambda'] = {lam} (finite and >= 0)")
    return {"maps": "calibrated", "calib": parse_calib(over.get("calib"), H, W),
            "baseline": parse_sense_baseline(over.get("baseline")), "cg_lambda": lam}


def prior_settings(config: dict) -> Optional[dict]:
    """config['sense']['prior']: None when absent or 'none', else sense_prior.parse_prior's {'kind': 'tv',
    'weight', 'eps'}.  Valid with learned and with calibrated maps.  ValueError for every refusal."""
    from .sense_prior import parse_prior
    over = _only(config.get("sense"), SENSE_KEYS + MAPS_KEYS + PRIOR_KEYS, "config['sense']")
    return parse_prior(over.get("prior"))


def calibration_mask(calib: dict, undersampling, shape, mask: Optional[torch.Tensor] = None, mask_seed=None):
    """maps: calibrated -- (mask, acceleration): the sampling mask [C*H*W] (bool, CPU) the fit runs under -- the caller's,
    or the one ``undersampling`` (config['undersampling']) draws as ResidentFit._resident_data would -- with the
    calibration block OR-ed into every coil (calib['acs']) or checked to be fully sampled (ValueError naming the number
    of missing entries), and numel / sampled of the result.  (None, 1.0) without any mask: the block is taken as it is."""
    from .sense_calib import add_acs, missing_in_block
    from .undersampling import Undersampler, parse_undersampling_argument
    C_, H, W = (int(v) for v in shape[:3])
    a, b = calib["size"]
    if mask is not None:
        m = mask.detach().cpu().reshape(C_, H, W).numpy() != 0
    else:
        method, uparams = parse_undersampling_argument(undersampling)
        if method is None or method.lower() == "none":
            return None, 1.0
        hw = Undersampler(method, seed=mask_seed).create_mask(H, W, uparams).cpu().numpy() != 0
        m = np.broadcast_to(hw[None], (C_, H, W))
    if calib["acs"]:
        m = np.stack([add_acs(m[c], a, b) for c in range(C_)])
    else:
        missing = missing_in_block(m, a, b)
        if missing:
            raise ValueError(f"config['sense']['calib']: the {a} x {b} centre block is not fully sampled under the mask: "
                             f"{missing} of its {C_ * a * b} entries (over {C_} coils) are missing; set acs: true to add "
                             "the block to the mask")
    acceleration = float(m.size / max(int(np.count_nonzero(m)), 1))
    return torch.from_numpy(np.ascontiguousarray(m).reshape(-1)), acceleration


def coil_groups(n_coils: int, per_step: int) -> list:
    """[(c0, c1)] of the steps of an epoch: consecutive coils, the last group smaller when per_step does not divide"""
    return [(c0, min(c0 + per_step, n_coils)) for c0 in range(0, n_coils, per_step)]


def sens_net_params(settings: dict, encoder_config: dict) -> dict:
    """the FFN parameters of the sensitivity network behind its encoder"""
    emb = encoder_config["embedding"]
    E = settings["encoder"]["embedding_size"]
    size = 2 * E if emb == "gauss" else E if emb == "LogF" else int(encoder_config.get("coordinates_size", 3))
    return {"network_input_size": size, "network_output_size": 2, "network_depth": settings["net"]["network_depth"],
            "network_width": settings["net"]["network_width"]}


def check_offgrid_sense_config(config: dict, mask=None) -> None:
    """config['trajectory'] in a SENSE fit: built for calibrated maps only, and -- as INRTrainer's
    off-grid fits -- with the trajectory as the only sampling.  Refused before any device call."""
    t = config["trajectory"]
    sense = config.get("sense")
    if not isinstance(sense, dict) or sense.get("maps", "learned") != "calibrated":
        raise NotImplementedError(f"config['trajectory'] = {t!r}: off-grid SENSE fits are built for sense.maps: calibrated "
                                  "only (with learned maps the step's transform is a plain FFT)")
    from .undersampling import parse_undersampling_argument
    method, _ = parse_undersampling_argument(config.get("undersampling"))
    if mask is not None or (method is not None and method.lower() != "none"):
        raise ValueError(f"trajectory = {t!r} with an undersampling pattern or a mask: the trajectory IS the sampling")
    if isinstance(sense.get("calib"), dict) and "acs" in sense["calib"]:
        raise ValueError(f"trajectory = {t!r} with config['sense']['calib']['acs']: an off-grid acquisition has no "
                         "Cartesian centre block to add; the maps are calibrated from the samples")
    if config.get("loss") == "HDR":
        raise NotImplementedError(f"trajectory = {t!r} with loss 'HDR': its scalar A over the off-grid rows is not built "
                                  "for SENSE fits")
    if config.get("trajectory_baseline") not in (None, "none"):
        raise ValueError(f"trajectory = {t!r} with config['trajectory_baseline']: the conventional reconstruction of a "
                         "SENSE fit is config['sense']['baseline'] = cg-N (non-Cartesian CG-SENSE)")


def sense_operator(config: dict) -> Optional[str]:
    """the operator pair of an off-grid SENSE step: None without a trajectory, else config['trajectory_operator'] with
    "gridding" as the default (elsewhere the key belongs to a baseline and defaults to "exact")"""
    from .trajectory import parse_operator
    if config.get("trajectory") in (None, "none"):
        return None
    return parse_operator(config.get("trajectory_operator")) or "gridding"


def check_sense_config(config: dict, world: int = 1, graph_steps: bool = False) -> None:
    """What a SENSE-model fit cannot be combined with -- refused before anything is allocated."""
    name = config["model"]
    if name in MFN_MODELS:
        raise NotImplementedError(f"model {name!r}: the image network of a SENSE-model fit is SIREN / FFN / WIRE / WIRE2D, "
                                  "not one of the filter networks")
    if name not in MODELS:
        raise NotImplementedError(f"model {name!r} has no MI355X kernel yet (have {sorted(set(MODELS) - set(MFN_MODELS))})")
    if config.get("optimizer", "Adam") != "Adam":
        raise NotImplementedError("only Adam")
    if config.get("transform", False):
        raise NotImplementedError("transform: true: a SENSE-model fit lives in image space already and is fitted to "
                                  "k-space data; image-space data have no sampling mask to profit from")
    if config["trajectory"] not in (None, "none"):
        check_offgrid_sense_config(config)
    if config.get("ring_normalization") not in (None, "none", False):
        raise NotImplementedError(f"config['ring_normalization'] = {config['ring_normalization']!r}: the targets of a "
                                  "SENSE-model fit stay in the data's units (the model is linear in image space)")
    if config.get("row_sampling") not in (None, "none", False):
        raise NotImplementedError(f"config['row_sampling'] = {config['row_sampling']!r}: a step transforms whole coil "
                                  "planes; weighted epochs run in INRTrainer (python -m inr_mi355x.train) only")
    if config["per_coil"] or config["use_tv"]:
        raise NotImplementedError("per_coil / use_tv: a SENSE-model step takes config['sense']['coils_per_step'] whole "
                                  "coils, and use_tv is the reference's TV of a coil's predicted k-space; the TV prior "
                                  "on the image is config['sense']['prior'] (sense.prior: {kind: tv, weight, eps})")
    if config.get("virtual_coils"):
        raise NotImplementedError(f"config['virtual_coils'] = {config['virtual_coils']!r}: compressed coils have no "
                                  "smooth sensitivity map over a coil coordinate")
    if config.get("loss") == "LSL":
        raise NotImplementedError("loss 'LSL' (CenterLoss): its random-pair term is not part of inr_loss_grad")
    if config.get("loss") == "FFL":
        raise NotImplementedError("loss 'FFL' (focal frequency loss): FFL fits run in INRTrainer (python -m "
                                  "inr_mi355x.train) only")
    if config["regularization"]["type"] != "none":
        raise NotImplementedError(f"regularization {config['regularization']['type']!r}: the penalty is over all "
                                  "parameters of both networks and would couple the two engines")
    if config.get("precision", "f32") != "f32":
        raise NotImplementedError(f"precision {config['precision']!r}: SENSE-model fits run the fp32 tier-1 calls")
    if graph_steps:
        raise NotImplementedError("graph_steps: a SENSE-model step is a sequence of tier-1 calls and FFTs on two plans")
    if world > 1:
        raise NotImplementedError("SENSE-model fits run on one rank")


def sens_stash_bytes(net_params: dict, gauss: bool, enc_size: int, rows: int) -> int:
    """bytes of the activation stash the sensitivity plan needs for a step of ``rows`` rows (inr_plan_launch_dims /
    inr_plan_workspace of a plan made for the question alone: nothing is allocated on the device)"""
    from .engine import MLPEngine
    eng = MLPEngine(L.KIND_FFN, net_params["network_input_size"], net_params["network_width"], net_params["network_depth"],
                    net_params["network_output_size"], L.ACT_SIGMOID, L.INPUT_GAUSS if gauss else L.INPUT_X,
                    enc_size if gauss else 0)
    return max(eng.launch_dims(rows)[0], eng.workspace(rows)[0]) * eng.save_floats_per_tile * 4


class SenseFitTrainer(ResidentFit):
    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, shape, device, seed: int = 0,
                 mask: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1, process_group=None,
                 mask_seed: Optional[int] = None, graph_steps: bool = False, coil_compression=None):
        C_, H, W = (int(v) for v in shape[:3])
        defaults = set_default_configs(dict(config))
        if coil_compression is not None:
            defaults["virtual_coils"] = defaults.get("virtual_coils") or coil_compression.coils_out
        check_sense_config(defaults, world, graph_steps)
        self.operator = sense_operator(defaults)  # None: Cartesian; "gridding" | "exact": off-grid
        if self.operator is not None:
            check_offgrid_sense_config(defaults, mask)
        self.settings = sense_settings(defaults, C_)
        self.calib = maps_settings(defaults, H, W)  # None: learned maps
        self.prior = prior_settings(defaults)  # None: no prior on the image
        emb = defaults["encoder"]["embedding"]
        G = self.coils_per_step = self.settings["coils_per_step"]
        if self.calib is None:
            if self.settings["encoder"]["embedding_size"] is None:
                raise ValueError("config['encoder']['embedding_size'] (or config['sense']['encoder']['embedding_size'])")
            self.sens_params = sens_net_params(self.settings, defaults["encoder"])
            self._check_stash(G, H * W, emb == "gauss")
        elif self.operator is not None:  # the trajectory is the sampling; the maps come from the samples (_ingest)
            self.acceleration = 1.0
            if G != C_:
                raise ValueError(f"config['sense']['coils_per_step'] = {G}: an off-grid step takes all {C_} coils")
        else:  # the mask with the calibration block in it, formed up front and handed on as the explicit mask
            mask, self.acceleration = calibration_mask(self.calib["calib"], defaults["undersampling"], (C_, H, W), mask,
                                                       mask_seed)
        config = dict(config)
        config.setdefault("batch_size", H * W)  # the step's batches are coil groups; the key is read by the base only
        config = self._init_fit(config, shape, device, seed, rank, world, process_group, False, None,
                                trajectory_ok=self.operator is not None, step_operator_ok=self.operator is not None)
        # encoder, image network, sensitivity encoder, sensitivity network: all on one CPU generator, in this order
        self._seeded_encoder(seed)
        model = MODELS[config["model"]](config["net"])
        if self.calib is not None:
            self.model = model.to(self.device)
            self.sens_encoder = self.sens_model = self.sens_engine = self.sens_enc_B = None
            self.engine, self.enc_B = mlp_engine(self.model, self.encoder, config["encoder"])
        else:
            self._two_networks(model, config)
        if self.engine.out_features != 2:
            raise ValueError(f"config['net']['network_output_size'] = {self.engine.out_features}: the image network gives "
                             "one complex number (2 outputs)")
        self.loss = LossSpec.from_config(config)
        # the base's shuffled epochs permute ROWS; here the order of the coil groups is permuted, as per-coil fits do
        shuffle, self.shuffle = self.shuffle, False
        self._resident_data(image, coords, config["undersampling"], mask, mask_seed, False)
        if self.calib is not None and self.mask is not None:  # an explicit mask leaves the data unmasked: zero-fill them
            self.image = (self.image_full * self.mask.view(-1, 1).to(self.image_full.dtype)).contiguous()
            self.train_values = self._train_values_data = self._t_image = self.image
        self.shuffle = shuffle
        self.plane = H * W
        self.groups = coil_groups(C_, G)
        self.bs = G * self.plane  # validation's test loss walks the same groups
        self.steps_per_epoch = len(self.groups)
        if self.shuffle and len(self.groups) > 1:
            self._coil_order = CoilOrder(len(self.groups), self.shuffle_seed)
        self._ingest(C_, H, W)
        self._last_sense = self._last_prior = None
        if self.prior is not None:  # the prior's value and block partials, made once
            self._prior_out = torch.zeros(L.LOSS_WORDS, device=self.device)
        self.cg_sense = self._cg_image = self._cg_rss = None
        self._finish_init()
        if self.calib is not None and self.calib["baseline"] is not None:
            self._cg_sense_offgrid_baseline() if self.operator is not None else self._cg_sense_baseline()

    # ---- set-up ----------------------------------------------------------------------------------
    def _two_networks(self, model, config: dict) -> None:
        """learned maps: the sensitivity encoder and network follow the image network on the same CPU generator"""
        sens_enc = sens_encoder_config(self.settings, config["encoder"])
        self.sens_encoder = Positional_Encoder(sens_enc, device=self.device)
        sens_model = FFN(self.sens_params)
        self.model, self.sens_model = model.to(self.device), sens_model.to(self.device)
        self.engine, self.enc_B = mlp_engine(self.model, self.encoder, config["encoder"])
        self.sens_engine, self.sens_enc_B = mlp_engine(self.sens_model, self.sens_encoder, sens_enc)

    def _check_stash(self, G: int, plane: int, gauss: bool) -> None:
        budget, E = self.settings["max_stash_bytes"], self.settings["encoder"]["embedding_size"]
        need = sens_stash_bytes(self.sens_params, gauss, E, G * plane)
        if need <= budget:
            return
        fits = next((g for g in range(G - 1, 0, -1) if sens_stash_bytes(self.sens_params, gauss, E, g * plane) <= budget), 0)
        hint = f"the largest that fits is coils_per_step = {fits}" if fits else "not even coils_per_step = 1 fits"
        raise ValueError(f"config['sense']['coils_per_step'] = {G}: the sensitivity plan's activation stash for {G} x "
                         f"{plane} rows is {need} bytes, config['sense']['max_stash_bytes'] = {budget}; {hint}")

    @torch.no_grad()
    def _ingest(self, C_: int, H: int, W: int) -> None:
        """Once: the inputs of both networks, the targets and the mask in ifftshift-ed row order per coil (what a plain
        fft2 of the product kernel's output is compared with), and the factor of the product."""
        if self.operator is not None:
            return self._ingest_offgrid(C_, H, W)
        perm = torch.from_numpy(shift_index(H, W)).to(self.device)
        self._gt_s = self.image.view(C_, self.plane, 2)[:, perm].contiguous().view(-1, 2)
        self._mask_s = None if self.mask is None else self.mask.view(C_, self.plane)[:, perm].contiguous().view(-1)
        self._img_coords = self.coords[:self.plane].clone()
        self._img_coords[:, 0] = 0.0
        self._img_in = _encoded(self.encoder, self.enc_B, self._img_coords)
        self.sense_scale = self.settings["scale"]
        if self.sense_scale is None:
            from .evalchain import ifft2c
            zf = ifft2c(self.image.view(C_, H, W, 2)).double()  # self.image: the zero-filled (masked) k-space
            if self.calib is None:
                self.sense_scale = float(torch.sqrt((zf ** 2).sum(-1).mean()))
            else:
                # unit-RSS maps leave the whole magnitude to the image network, whose last_tanh bounds it by 1: the
                # largest RSS of the zero-filled images, times the acceleration (zero-filling with a fraction 1/R of the
                # entries shows the object at 1/R of its magnitude, plus aliases)
                self.sense_scale = float(torch.sqrt((zf ** 2).sum(dim=(0, 3)).max())) * self.acceleration
            if not math.isfinite(self.sense_scale):
                raise ValueError(f"the RMS of the zero-filled coil images is {self.sense_scale}")
            if self.sense_scale == 0.0:
                self.sense_scale = 1.0
        self._x = torch.empty(self.coils_per_step, H, W, 2, device=self.device)
        if self.calib is not None:
            from .sense_calib import calibrate, cut_block
            c = self.calib["calib"]
            self._block = torch.from_numpy(cut_block(self.image.view(C_, H, W, 2), *c["size"], c["window"])).to(self.device)
            self._maps, self.sens_rss = calibrate(self._block, H, W, c["floor"])  # [C,P,2], [P]: resident
            self._maps_rows = self._maps.view(-1, 2)
            self._dimg = torch.empty(self.plane, 2, device=self.device)
            stats = torch.stack((self.sens_rss.min(), self.sens_rss.max(), self.sens_rss.double().mean().float()))
            self._rss_stats = dict(zip(("min", "max", "mean"), stats.cpu().tolist()))

    @torch.no_grad()
    def _ingest_offgrid(self, C_: int, H: int, W: int) -> None:
        """Once, for an off-grid fit: the targets are the [C, M, 2] samples _resident_data took (the exact
        NUDFT of the coil images).  Everything else comes from those samples alone: their density-weighted exact adjoint
        gives coil images whose largest RSS is the default factor (the weights sum to H W: no acceleration factor) and
        whose centred k-space gives the calibration block; from the block on, the Cartesian path's calibrate()."""
        from .evalchain import fft2c
        from .sense_calib import calibrate, cut_block
        from .sense_nufft import SenseNufft
        from .trajectory import (adjoint_scratch_floats, nudft_adjoint, parse_density, positions, scratch_floats,
                                 _device_positions)
        self.plane = H * W
        self._gt_s = self._mask_s = None
        self._pos = positions(self.trajectory, H, W)
        self.M = int(self._pos.shape[0])
        self._gt = self._train_values_data  # [(C*M), 2]
        self.density_name, w = parse_density(self.config["trajectory_density"], self.trajectory, H, W)
        self._img_coords = self.coords[:self.plane].clone()
        self._img_coords[:, 0] = 0.0
        self._img_in = _encoded(self.encoder, self.enc_B, self._img_coords)
        back = nudft_adjoint(self._gt.view(C_, self.M, 2), self._pos, (H, W), w)  # [C,H,W,2]
        self.sense_scale = self.settings["scale"]
        if self.sense_scale is None:
            self.sense_scale = float(torch.sqrt((back.double() ** 2).sum(dim=(0, 3)).max()))
            if not math.isfinite(self.sense_scale):
                raise ValueError(f"the largest RSS of the adjoint coil images is {self.sense_scale}")
            if self.sense_scale == 0.0:
                self.sense_scale = 1.0
        c = self.calib["calib"]
        self._block = torch.from_numpy(cut_block(fft2c(back), *c["size"], c["window"])).to(self.device)
        self._maps, self.sens_rss = calibrate(self._block, H, W, c["floor"])
        self._maps_rows = self._maps.view(-1, 2)
        self._x = torch.empty(C_, H, W, 2, device=self.device)  # the prediction sweep's coil images; the exact step's
        self._dimg = torch.empty(self.plane, 2, device=self.device)
        stats = torch.stack((self.sens_rss.min(), self.sens_rss.max(), self.sens_rss.double().mean().float()))
        self._rss_stats = dict(zip(("min", "max", "mean"), stats.cpu().tolist()))
        self._op = None  # the fused pair's buffers: the gridding step's, and the CG baseline's under either operator
        if self.operator == "gridding" or self.calib["baseline"] is not None:
            self._op = SenseNufft(self._maps, self._pos, (C_, H, W), self.sense_scale, w)
        if self.operator == "exact":
            self._pos_dev = _device_positions(self._pos, self.device)
            self._scratch_fwd = torch.empty(scratch_floats(C_, H, W, self.M), device=self.device)
            self._scratch_adj = torch.empty(adjoint_scratch_floats(C_, H, W, self.M), device=self.device)
            self._gx = torch.empty(C_, H, W, 2, device=self.device)

    def _step_offgrid(self, epoch: int) -> torch.Tensor:
        """forward -> E -> inr_loss_grad on [G*M, 2] -> E^H -> prior -> backward -> Adam, all coils.  E is the fused
        gridding pair (sense_nufft.py), or under trajectory_operator: exact the existing kernels alone --
        inr_sense_apply(shift 0) -> inr_nudft and inr_adjoint_nudft -> inr_sense_adjoint(shift 0): slow, and the yardstick."""
        C_, H, W = (int(v) for v in self.shape[:3])
        cfg, lr = self.config, self._lr(epoch)
        ib = self.engine.forward(self._img_in, self.enc_B, save=True)
        if self.operator == "gridding":
            k = self._op.forward(ib)
        else:
            from .trajectory import nudft
            x = sense_apply(ib, self._maps_rows, C_, H, W, self.sense_scale, 0, out=self._x)
            k = nudft(x, self._pos_dev, scratch=self._scratch_fwd)
        loss, gk = self.engine.loss_grad(self.loss, k.view(-1, 2), self._gt, C_ * self.M)
        if self.operator == "gridding":
            dimg = self._op.adjoint(gk.view(C_, self.M, 2), dimg=self._dimg)
        else:
            from .sense_calib import sense_adjoint
            from .trajectory import nudft_adjoint
            gx = nudft_adjoint(gk.view(C_, self.M, 2), self._pos_dev, (H, W), None, scratch=self._scratch_adj, out=self._gx)
            dimg = sense_adjoint(self._maps_rows, gx, C_, H, W, self.sense_scale, 0, dimg=self._dimg)
        if self.prior is not None:
            loss = loss + self._add_prior(ib, dimg, H, W)
        self.engine.backward(self._img_in, self.enc_B, dimg)
        self.engine.adam_step(lr, cfg["beta1"], cfg["beta2"], 1e-8, cfg["weight_decay"])
        self.global_step += 1
        return loss

    def _sens_in(self, lo: int, hi: int) -> torch.Tensor:
        return _encoded(self.sens_encoder, self.sens_enc_B, self.coords[lo:hi])

    # ---- one optimizer step ----------------------------------------------------------------------
    def _parts(self):
        """the image network; with learned maps the sensitivity network behind it, its encoder travelling with it"""
        parts = [Part(IMAGE_PREFIX, self.model, self.engine, self.encoder, self._rebind_encoder)]
        if self.calib is None:
            parts.append(Part(SENS_PREFIX, self.sens_model, self.sens_engine, self.sens_encoder, self._rebind_sens_encoder))
        return parts

    def step(self, epoch: int, it: int) -> torch.Tensor:
        if self.operator is not None:
            return self._step_offgrid(epoch)
        if self._coil_order is not None:
            it = self._coil_order.at(epoch, it)
        c0, c1 = self.groups[it]
        G, H, W = c1 - c0, int(self.shape[1]), int(self.shape[2])
        lo, hi = c0 * self.plane, c1 * self.plane
        count = max(self._count(lo, hi), 1)
        A = self._batch_hdr_A(it, lo, hi)
        cfg, lr = self.config, self._lr(epoch)
        m = None if self._mask_s is None else self._mask_s[lo:hi]
        if self.calib is not None:
            from .sense_calib import sense_adjoint
            ib = self.engine.forward(self._img_in, self.enc_B, save=True)
            x = sense_apply(ib, self._maps_rows[lo:hi], G, H, W, self.sense_scale, 1, out=self._x[:G])
            k = torch.view_as_real(torch.fft.fft2(torch.view_as_complex(x), norm="ortho"))
            loss, gk = self.engine.loss_grad(self.loss, k.view(-1, 2), self._gt_s[lo:hi], count, mask=m, hdr_A=A)
            gx = torch.view_as_real(torch.fft.ifft2(torch.view_as_complex(gk.view(G, H, W, 2)), norm="ortho"))
            dimg = sense_adjoint(self._maps_rows[lo:hi], gx, G, H, W, self.sense_scale, 1, dimg=self._dimg)
            if self.prior is not None:
                loss = loss + self._add_prior(ib, dimg, H, W)
            self.engine.backward(self._img_in, self.enc_B, dimg)
            self.engine.adam_step(lr, cfg["beta1"], cfg["beta2"], 1e-8, cfg["weight_decay"])
            self.global_step += 1
            return loss
        xs = self._sens_in(lo, hi)
        ib = self.engine.forward(self._img_in, self.enc_B, save=True)
        sb = self.sens_engine.forward(xs, self.sens_enc_B, save=True)
        x = sense_apply(ib, sb, G, H, W, self.sense_scale, 1, out=self._x[:G])
        k = torch.view_as_real(torch.fft.fft2(torch.view_as_complex(x), norm="ortho"))
        loss, gk = self.engine.loss_grad(self.loss, k.view(-1, 2), self._gt_s[lo:hi], count, mask=m, hdr_A=A)
        gx = torch.view_as_real(torch.fft.ifft2(torch.view_as_complex(gk.view(G, H, W, 2)), norm="ortho"))
        dimg, dsens = sense_grad(ib, sb, gx, G, H, W, self.sense_scale, 1)
        if self.prior is not None:  # every group's step carries the prior with its full weight
            loss = loss + self._add_prior(ib, dimg, H, W)
        self.engine.backward(self._img_in, self.enc_B, dimg)
        self.sens_engine.backward(xs, self.sens_enc_B, dsens)
        for part in self._parts():
            part.engine.adam_step(lr, cfg["beta1"], cfg["beta2"], 1e-8, cfg["weight_decay"])
        self.global_step += 1
        return loss

    def _add_prior(self, ib: torch.Tensor, dimg: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """weight * dTV/dI of the image network's output ``ib`` added into ``dimg`` (inr_image_tv_grad, accumulate);
        returns weight * TV, a view of the prior's resident loss_out buffer.  The prior acts on I, not on scale * I."""
        from .sense_prior import image_tv
        return image_tv(ib, H, W, self.prior["weight"], self.prior["eps"], dimg=dimg, accumulate=True,
                        loss_out=self._prior_out)

    # ---- validation ------------------------------------------------------------------------------
    def _sweep(self, engine, enc_B, rows: torch.Tensor, chunk: int, encoder) -> torch.Tensor:
        n = rows.shape[0]
        return torch.cat([engine.forward(_encoded(encoder, enc_B, rows[lo:min(lo + chunk, n)]), enc_B, save=False)
                          for lo in range(0, n, chunk)], 0)

    @torch.no_grad()
    def _predict_raw(self, chunk: Optional[int] = None) -> torch.Tensor:
        """k-space [C*H*W,2] in the dataset's own order, without a stash: the image network once, then group by group (the
        step's coil groups, so that beside the prediction itself only one group's sensitivities and coil images exist at
        a time) the sensitivity network in chunks of rows, inr_sense_apply(shift = 1), fft2, fftshift.  Leaves sens_rss
        behind.  reconstruct.Reconstructor sweeps and transforms in the same groups: a forward call's bits depend on how
        the rows are cut into calls."""
        chunk = int(chunk or self.predict_chunk)
        C_, H, W = (int(v) for v in self.shape[:3])
        img = self._sweep(self.engine, self.enc_B, self._img_coords, chunk, self.encoder)
        if self.prior is not None:  # the prior's value on the swept image: no gradient, one host read
            from .sense_prior import image_tv
            value = image_tv(img, H, W, self.prior["weight"], self.prior["eps"], loss_out=self._prior_out)
            self._last_prior = dict(self.prior, value=float(value))
        out = torch.empty(C_, H, W, 2, device=self.device)
        if self.calib is not None:  # the same sweep through the resident maps
            for c0, c1 in self.groups:
                x = sense_apply(img, self._maps_rows[c0 * self.plane:c1 * self.plane], c1 - c0, H, W, self.sense_scale, 1,
                                out=self._x[:c1 - c0])
                k = torch.fft.fftshift(torch.fft.fft2(torch.view_as_complex(x), norm="ortho"), dim=(-2, -1))
                out[c0:c1] = torch.view_as_real(k)
            self._last_sense = {"coils_per_step": self.coils_per_step, "scale": self.sense_scale, "maps": "calibrated",
                                "calib": dict(self.calib["calib"], acceleration=self.acceleration),
                                "sens_rss": dict(self._rss_stats)}
            return out.view(-1, 2)
        rss2 = torch.zeros(self.plane, dtype=torch.float64, device=self.device)
        for c0, c1 in self.groups:
            G = c1 - c0
            sens = self._sweep(self.sens_engine, self.sens_enc_B, self.coords[c0 * self.plane:c1 * self.plane], chunk,
                               self.sens_encoder)
            rss2 += (sens.double() ** 2).view(G, self.plane, 2).sum(dim=(0, 2))
            x = sense_apply(img, sens, G, H, W, self.sense_scale, 1, out=self._x[:G])
            k = torch.fft.fftshift(torch.fft.fft2(torch.view_as_complex(x), norm="ortho"), dim=(-2, -1))
            out[c0:c1] = torch.view_as_real(k)
        rss = torch.sqrt(rss2)
        stats = torch.stack((rss.min(), rss.max(), rss.mean())).cpu().tolist()
        self._last_sense = {"coils_per_step": self.coils_per_step, "scale": self.sense_scale,
                            "net": {"width": self.sens_params["network_width"], "depth": self.sens_params["network_depth"]},
                            "sens_rss": {"min": stats[0], "max": stats[1], "mean": stats[2]}}
        return out.view(-1, 2)

    @property
    def sense_summary(self) -> Optional[dict]:
        """{'coils_per_step', 'scale', 'net': {'width', 'depth'}, 'sens_rss': {'min', 'max', 'mean'}} of the last sweep
        (None before the first).  Off-grid fits add which pair the step runs and where the block came
        from: 'operator', and 'calib' with source "samples" and the density's name in place of 'acs' / 'acceleration'."""
        if self.operator is None or self._last_sense is None:
            return self._last_sense
        calib = {k: v for k, v in self.calib["calib"].items() if k != "acs"}
        return dict(self._last_sense, operator=self.operator, calib=dict(calib, source="samples", density=self.density_name))

    @torch.no_grad()
    def validate(self, epoch: int) -> dict:
        rec = self._validated(epoch, self._predict_raw())
        rec["sense"] = self.sense_summary
        if self.prior is not None:
            rec["prior"] = self._last_prior
        if self.cg_sense is not None:
            rec["cg_sense"] = self.cg_sense
        return rec

    @torch.no_grad()
    def metrics(self) -> dict:
        rec = super().metrics()
        rec["sense"] = self.sense_summary
        if self.prior is not None:
            rec["prior"] = self._last_prior
        if self.cg_sense is not None:
            rec["cg_sense"] = self.cg_sense
        return rec

    # ---- the conventional reconstruction from the same maps and samples ---------------------------
    @torch.no_grad()
    def _cg_sense_baseline(self) -> None:
        """config['sense']['baseline'] = cg-N: N conjugate-gradient iterations of CG-SENSE
        (sense_calib.cg_sense) on the fit's own maps, samples and mask, made once; its k-space prediction is scored as
        the fit's own is (coil images, RSS, PSNR / SSIM against the full data through the validation's kernel).  Leaves
        the record in self.cg_sense, the image [H*W,2] in self._cg_image and its RSS picture in self._cg_rss; reads no
        random number and no parameter."""
        import time
        from .evalchain import image_metrics
        from .sense_calib import cg_sense, kspace_of
        from .validation import coil_images
        iters, lam = self.calib["baseline"], self.calib["cg_lambda"]
        torch.cuda.synchronize(self.device)
        t0 = time.time()
        iterates, objective = cg_sense(self._maps, self._gt_s, self._mask_s, self.shape, iters, lam)
        self._cg_image = iterates[-1].contiguous()
        torch.cuda.synchronize(self.device)
        seconds = time.time() - t0
        pred = kspace_of(self._cg_image, self._maps, self.shape)
        if self._ref_rss is None:
            self._ref_rss = image_metrics(None, coil_images(self.image_full, self.shape, self.in_image_space))[0]
        self._cg_rss, m = image_metrics(self._ref_rss, coil_images(pred, self.shape, self.in_image_space))[:2]
        psnr_, ssim_ = m[:2].cpu().tolist()
        self.cg_sense = {"iters": iters, "lambda": lam, "psnr": psnr_, "ssim": ssim_,
                         "objective": [float(v) for v in objective], "seconds": seconds}

    @torch.no_grad()
    def _cg_sense_offgrid_baseline(self) -> None:
        """config['sense']['baseline'] = cg-N of an off-grid fit: non-Cartesian CG-SENSE (Pruessmann 2001),
        N iterations on (E^H W E + lambda) x = E^H W y with E the fused gridding pair at scale 1 and W the density weights
        (sense_nufft.cg_sense_offgrid), from the fit's own maps and samples; scored and kept as the Cartesian baseline is."""
        import time
        from .evalchain import image_metrics
        from .sense_calib import kspace_of
        from .sense_nufft import cg_sense_offgrid
        from .validation import coil_images
        iters, lam = self.calib["baseline"], self.calib["cg_lambda"]
        C_ = int(self.shape[0])
        torch.cuda.synchronize(self.device)
        t0 = time.time()
        iterates, objective = cg_sense_offgrid(self._op, self._gt.view(C_, self.M, 2), iters, lam)
        self._cg_image = iterates[-1].contiguous()
        torch.cuda.synchronize(self.device)
        seconds = time.time() - t0
        pred = kspace_of(self._cg_image, self._maps, self.shape)
        if self._ref_rss is None:
            self._ref_rss = image_metrics(None, coil_images(self.image_full, self.shape, self.in_image_space))[0]
        self._cg_rss, m = image_metrics(self._ref_rss, coil_images(pred, self.shape, self.in_image_space))[:2]
        psnr_, ssim_ = m[:2].cpu().tolist()
        self.cg_sense = {"iters": iters, "lambda": lam, "psnr": psnr_, "ssim": ssim_,
                         "objective": [float(v) for v in objective], "seconds": seconds, "operator": "gridding",
                         "density": self.density_name}

    @torch.no_grad()
    def save_cg_sense_image(self, directory: str, prefix: str = "") -> str:
        """cg_sense_{psnr}_psnr_{ssim}_ssim.png: the baseline's RSS image through the display kernels"""
        import os
        if self.cg_sense is None:
            raise RuntimeError("save_cg_sense_image: the fit has no config['sense']['baseline']")
        D, b = self._display()
        os.makedirs(directory, exist_ok=True)
        name = prefix + "cg_sense_{:.4g}_psnr_{:.4g}_ssim.png".format(self.cg_sense["psnr"], self.cg_sense["ssim"])
        return self._write_gray(D, b, os.path.join(directory, name), self._cg_rss, True)

    # ---- checkpoints -----------------------------------------------------------------------------
    def _sense_state(self) -> dict:
        if self.calib is not None:
            from .sense_calib import calibrated_state
            state = calibrated_state(self.sense_scale, self.coils_per_step, self.calib["calib"], self._block)
        else:
            state = {"scale": self.sense_scale, "coils_per_step": self.coils_per_step,
                     "enc_B": None if self.sens_encoder.B is None else self.sens_encoder.B.clone(),
                     "net": dict(self.settings["net"]), "encoder": dict(self.settings["encoder"])}
        if self.prior is not None:  # a record only: resuming under another weight is allowed, as for lr
            state["prior"] = dict(self.prior)
        return state

    def checkpoint(self) -> dict:
        """{'net', 'enc', 'opt'} in the reference's layout -- 'net' with 'image.*' then 'sens.*' keys, 'enc' the image
        network's encoder matrix, 'opt' in torch.optim.Adam.state_dict() layout over the image network's parameters, then
        the sensitivity network's -- plus 'sense': the factor, the sensitivity encoder's matrix and the sizes."""
        parts = self._parts()  # calibrated maps: 'image.*' alone; the maps are not stored, 'sense' holds their block
        return {"net": joined_net(parts), "enc": None if self.encoder.B is None else self.encoder.B.clone(),
                "opt": joined_optimizer_state(parts, self.config), "sense": self._sense_state()}

    def _rebind_sens_encoder(self, enc) -> None:
        if self.sens_enc_B is not None:
            self.sens_enc_B = enc.B.contiguous()

    def load_checkpoint(self, ckpt: dict) -> None:
        """Resumes under the same ``sense`` settings only: factor, coils_per_step and both sizes must be the trainer's."""
        if not has_sense_keys(ckpt["net"]) or ckpt.get("sense") is None:
            raise ValueError("the checkpoint has no 'image.' / 'sens.' keys: it is not a SENSE-model fit's -- load it with "
                             "the trainer that wrote it")
        theirs, mine = ckpt["sense"], self._sense_state()
        from .sense_calib import check_calibrated_state, check_sense_mode, image_net_of
        check_sense_mode(theirs, "learned" if self.calib is None else "calibrated")
        if self.calib is not None:
            check_calibrated_state(theirs, mine)
            nets = [image_net_of(ckpt["net"])]
        else:
            for key in ("scale", "coils_per_step", "net", "encoder"):
                if theirs.get(key) != mine[key]:
                    raise ValueError(f"checkpoint and trainer disagree on config['sense']: {key} = {theirs.get(key)!r} in "
                                     f"the checkpoint, {mine[key]!r} here")
            nets = split_state(ckpt["net"])
        load_parts(self._parts(), nets, [ckpt.get("enc"), theirs.get("enc_B")][:len(nets)], ckpt.get("opt"))
        self._img_in = _encoded(self.encoder, self.enc_B, self._img_coords)  # the encoder may have been replaced


def add_sense_flags(ap) -> None:
    ap.add_argument("--sense-maps", type=str, default=None, metavar="ARG",
                    help="learned | calibrated (config['sense']['maps']): coil maps from a second network, or estimated "
                         "once from the fully sampled centre of k-space and fixed")
    ap.add_argument("--sense-prior", type=str, default=None, metavar="ARG",
                    help="none | tv:WEIGHT[:EPS] (config['sense']['prior']): smoothed isotropic total variation of the "
                         "image network's output, added to every step's loss with this weight (eps defaults to 1e-3)")
    ap.add_argument("--sense-baseline", type=str, default=None, metavar="ARG",
                    help="none | cg-N (config['sense']['baseline']; with calibrated maps): CG-SENSE from the same maps and "
                         "samples, scored as the fit is")


def apply_sense_flags(config: dict, opts) -> dict:
    from .sense_prior import parse_prior_flag
    prior = parse_prior_flag(getattr(opts, "sense_prior", None))
    for key, value in (("maps", opts.sense_maps), ("baseline", opts.sense_baseline), ("prior", prior)):
        if value is not None:
            config["sense"] = dict(config.get("sense") or {}, **{key: value})
    return config


def main():
    opts, config = parse_cli(extra_flags=add_sense_flags)
    config = apply_sense_flags(config, opts)
    for cfg, fit_opts in cli_fits(config, opts):
        image, coords, shape, cc = cli_fit_data(opts, cfg, "coil", image_space=False)
        tr = SenseFitTrainer(cfg, image, coords, shape, "cuda", coil_compression=cc)
        run_cli(tr, cfg, fit_opts, extra=None if tr.cg_sense is None else {"cg_sense": tr.cg_sense})


if __name__ == "__main__":
    main()
