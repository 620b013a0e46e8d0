"""Per-ring model ensemble: one network per k-means ring of k-space (the reference's
train_variations/train_clustering.py:121-190 over clustering.partition_kspace), mapped ONE RING PER GPU.

Ring i = coordinates with radii[i] <= dist <= radii[i+1] (both ends included, so boundary points belong to two
rings; at evaluation the outer ring's prediction wins, as the sequential ``batch_rec[ind] = output`` of the
reference, :199-211).  Every model sees every batch and trains on the rows of its ring: forward on all rows, loss
on the ring's rows, mean over the ring's rows (train_clustering.py:170-183) -- which is exactly the fused step
with a row mask.

Parallel mapping: ring i is owned by rank i % world.  Models are independent, so there is NO collective in
training; the evaluation sweep adds the ranks' disjoint contributions with one SUM all-reduce.

Kept different from the stale reference script, on purpose: batches are the sequential unshuffled ranges of the
maintained loops (the script shuffles; ``config["shuffle"]`` opts into the keyed per-epoch permutation of
inr_mi355x/shuffle.py -- not the script's DataLoader order, which nothing pins down), and the +-N(0, 0.05) jitter of the ring bounds (:166-167, an unseeded numpy
draw per model per step) is off by default and seeded when enabled.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .engine import LossSpec
from .evalchain import psnr, reconstruct
from .networks import Positional_Encoder
from .shuffle import EpochBuffers, shuffle_settings
from .train import MODELS, MFN_MODELS, lr_factor, set_default_configs
from .validation import ValidationMixin


def ring_owner(i: int, world: int) -> int:
    return i % world


def winning_ring(dist: torch.Tensor, radii: Sequence[float]) -> torch.Tensor:
    """Index of the LAST ring containing each point (-1: none), i.e. the one whose output survives the
    sequential overwrite of train_clustering.py:199-211."""
    win = torch.full(dist.shape, -1, dtype=torch.int64, device=dist.device)
    for i in range(len(radii) - 1):
        win[(dist >= radii[i]) & (dist <= radii[i + 1])] = i
    return win


class RingEnsembleTrainer(ValidationMixin):
    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, shape, device,
                 radii: Optional[Sequence[float]] = None, seed: int = 0, rank: int = 0, world: int = 1,
                 process_group=None, jitter: float = 0.0):
        config = set_default_configs(dict(config))
        self.shuffle, self.shuffle_seed = shuffle_settings(config, seed)
        self.config, self.device = config, torch.device(device)
        self.rank, self.world, self.pg = rank, world, process_group
        self.shape = shape
        if config["model"] not in MODELS or config["model"] in MFN_MODELS:
            raise NotImplementedError(f"ring ensembles are built from SIREN / FFN / WIRE / WIRE2D, not {config['model']!r}")
        C, H, W = int(shape[0]), int(shape[1]), int(shape[2])
        if radii is None:  # train_clustering.py:121-126
            from .clustering import partition_kspace
            part = config["partition"]
            _, radii = partition_kspace(image.to(self.device).reshape(C, H, W, 2),
                                        coords.to(self.device).reshape(C, H, W, 3),
                                        no_steps=part["no_steps"], no_parts=part["no_models"])
        self.radii = [float(r) for r in radii]
        self.no_models = len(self.radii) - 1
        self.owned = [i for i in range(self.no_models) if ring_owner(i, world) == rank]
        # one shared encoder, then the models in ring order: every rank builds ALL of them so that the RNG stream
        # (and therefore each ring's initial weights) does not depend on the world size; only owned ones move to HBM
        torch.manual_seed(seed)
        self.encoder = Positional_Encoder(config["encoder"], device=self.device)
        emb = config["encoder"]["embedding"]
        self.enc_B = self.encoder.B.contiguous() if emb == "gauss" else None
        self.models, self.engines = {}, {}
        for i in range(self.no_models):
            m = MODELS[config["model"]](config["net"])
            if i in self.owned:
                m = m.to(self.device)
                self.models[i] = m
                self.engines[i] = (m.fused_engine(config["encoder"]["embedding_size"]) if emb == "gauss"
                                   else m._engine())
        self.loss = LossSpec.from_config(config)
        self.n = coords.shape[0]
        self.coords = coords.to(self.device).contiguous()
        self.image = image.to(self.device).contiguous()
        self._init_validation()
        self.dist = torch.sqrt(self.coords[:, 1] ** 2 + self.coords[:, 2] ** 2)
        self.bs = int(config["batch_size"])
        self.steps_per_epoch = math.ceil(self.n / self.bs)
        self.global_step = 0
        self.jitter = float(jitter)
        self._rng = np.random.RandomState(seed)
        self._masks = {}
        # config['shuffle']: batches are views of the epoch buffers (every rank fills its own with the same order);
        # predict_all / evaluate / metrics keep reading the unshuffled data
        self._epoch_buf = None
        self._t_coords, self._t_image, self._t_dist = self.coords, self.image, self.dist
        if self.shuffle:
            self._epoch_buf = EpochBuffers(self.shuffle_seed, self.bs, self.coords, self.image)
            self._t_coords, self._t_image = self._epoch_buf.coords, self._epoch_buf.image

    def _inputs(self, lo: int, hi: int, train: bool = False):
        coords = self._t_coords if train else self.coords
        emb = self.config["encoder"]["embedding"]
        if self.enc_B is not None or emb == "none":
            return coords[lo:hi]
        return self.encoder.embedding(coords[lo:hi])

    def _begin_shuffled(self, epoch: int) -> None:
        """First step of a shuffled epoch: refill the epoch buffers, then every ring's row mask over the whole buffer and
        its per-batch counts -- one batched op and one read-back (the cached masks are tied to the batches' contents)."""
        if not self._epoch_buf.begin(epoch):
            return
        c = self._t_coords
        self._t_dist = d = torch.sqrt(c[:, 1] ** 2 + c[:, 2] ** 2)
        self._masks = {}
        if self.jitter > 0.0:
            return
        masks = torch.stack([((d >= self.radii[i]) & (d <= self.radii[i + 1])).to(torch.uint8)
                             for i in range(self.no_models)])
        counts = self._epoch_buf.batch_sums(masks).tolist()
        for i in range(self.no_models):
            for b in range(self._epoch_buf.n_batches):
                lo = b * self.bs
                self._masks[(i, lo)] = (masks[i, lo:min(lo + self.bs, self.n)], counts[i][b])

    def _ring_mask(self, i: int, lo: int, hi: int):
        r0, r1 = self.radii[i], self.radii[i + 1]
        if self.jitter > 0.0:  # train_clustering.py:166-167 (every rank draws for every ring: same stream everywhere)
            r0 = max(0.0, r0 - abs(self._rng.normal(0, self.jitter)))
            r1 = r1 + abs(self._rng.normal(0, self.jitter))
            d = self._t_dist[lo:hi]
            m = ((d >= r0) & (d <= r1)).to(torch.uint8)
            return m, int(m.sum())
        key = (i, lo)
        if key not in self._masks:
            d = self._t_dist[lo:hi]
            m = ((d >= r0) & (d <= r1)).to(torch.uint8).contiguous()
            self._masks[key] = (m, int(m.sum()))
        return self._masks[key]

    def step(self, epoch: int, it: int) -> List[Optional[float]]:
        """One batch through every owned ring model; returns the per-ring losses (None: ring absent from the batch)."""
        if self.shuffle:
            self._begin_shuffled(epoch)
        lo, hi = it * self.bs, min((it + 1) * self.bs, self.n)
        lr = self.config["lr"] * lr_factor(epoch, self.config["max_epoch"])
        x, gt = self._inputs(lo, hi, True), self._t_image[lo:hi]
        out: List[Optional[torch.Tensor]] = [None] * self.no_models
        for i in range(self.no_models):
            mask, cnt = self._ring_mask(i, lo, hi)  # drawn for every ring to keep the jitter stream rank-independent
            if i not in self.engines or cnt == 0:  # train_clustering.py:169: empty ring -> optimizer has nothing to do
                continue
            eng = self.engines[i]
            out[i] = eng.train_step(x, self.enc_B, gt, self.loss, count=cnt, mask=mask).clone()
            eng.adam_step(lr, self.config["beta1"], self.config["beta2"], 1e-8, self.config["weight_decay"])
        self.global_step += 1
        return out

    def fit(self, max_steps: Optional[int] = None, log_every: int = 0):
        logged = []
        for epoch in range(self.config["max_epoch"]):
            for it in range(self.steps_per_epoch):
                if max_steps is not None and self.global_step >= max_steps:
                    return logged
                losses = self.step(epoch, it)
                if log_every and self.global_step % log_every == 0:
                    logged.append((self.global_step, [None if l is None else float(l) for l in losses]))
        return logged

    @torch.no_grad()
    def predict_all(self, chunk: int = 1 << 17) -> torch.Tensor:
        """[N,2] reconstruction: each point from the last ring that contains it (train_clustering.py:199-211);
        ranks contribute their rings' rows and one SUM all-reduce assembles the whole."""
        rec = torch.zeros(self.n, 2, device=self.device)
        win = winning_ring(self.dist, self.radii)
        for lo in range(0, self.n, chunk):
            hi = min(lo + chunk, self.n)
            x = self._inputs(lo, hi)
            for i in self.owned:
                sel = win[lo:hi] == i
                if bool(sel.any()):
                    o = self.engines[i].forward(x, self.enc_B, save=False)
                    rec[lo:hi][sel] = o[sel]
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=self.pg)
        return rec

    @torch.no_grad()
    def evaluate(self) -> float:
        in_image_space = bool(self.config.get("transform", False))
        ref = reconstruct(self.image, self.shape, in_image_space)
        return float(psnr(ref, reconstruct(self.predict_all(), self.shape, in_image_space)))

    def _display_source(self):
        return self.image, bool(self.config.get("transform", False))

    @torch.no_grad()
    def metrics(self) -> dict:
        """PSNR and SSIM of the assembled reconstruction on the device (the reference's ring loop has no validation
        epoch, hence no test loss).  Every rank that calls it after the all-reduce of predict_all gets the same numbers."""
        m = self._device_metrics(self.image, self.predict_all(), bool(self.config.get("transform", False)))
        psnr_, ssim_ = m[:2].cpu().tolist()
        return {"psnr": psnr_, "ssim": ssim_}

    def checkpoints(self) -> dict:
        """{ring: {'net', 'enc'}} of the owned rings (submodel_%d files of train_clustering.py:243-249)."""
        return {i: {"net": self.models[i].state_dict(), "enc": self.encoder.B} for i in self.owned}


def main():
    """python -m inr_mi355x.train_ring_ensemble --config cfg.yaml [--output_path out] [--synthetic C,H,W]
    [--max_steps N] [--shuffle] [--shuffle-seed S] [--save-images]: fit the rings (radii from config['partition']), print
    one JSON line with the assembled reconstruction's PSNR / SSIM and save the submodel_%d files of
    train_clustering.py:243-249.  --save-images writes train.png / train_kspace.png and the final metrics()' pictures
    to <output_path>/images (the ring loop has no validation epoch), the submodels to <output_path>/checkpoints, and
    prints the per-coil table."""
    import argparse
    import json
    import os
    import time

    from .synthetic import make_kspace
    from .train import add_image_flags, add_shuffle_flags, apply_shuffle_flags, get_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--output_path", type=str, default=".")
    ap.add_argument("--synthetic", type=str, default=None,
                    help="C,H,W: fit a synthetic k-space of that shape instead of the scan the config names")
    ap.add_argument("--max_steps", type=int, default=None)
    add_shuffle_flags(ap)
    add_image_flags(ap)
    opts = ap.parse_args()
    config = apply_shuffle_flags(set_default_configs(get_config(opts.config)), opts)
    if opts.synthetic:
        C, H, W = (int(v) for v in opts.synthetic.split(","))
        image, coords, shape = make_kspace(C, H, W, normalization=config.get("normalization", "coil"),
                                           image_space=bool(config.get("transform", False)))
    else:
        from .datasets import from_config, trainer_inputs
        image, coords, shape = trainer_inputs(from_config(config, "cuda"))
    tr = RingEnsembleTrainer(config, image, coords, shape, "cuda")
    os.makedirs(opts.output_path, exist_ok=True)
    ckpt_dir, image_dir = opts.output_path, None
    if opts.save_images:
        from .display import coil_stats_table, prepare_sub_folder
        ckpt_dir, image_dir = prepare_sub_folder(opts.output_path)
        tr.enable_validation_images()
        tr.save_training_images(image_dir)
    t0 = time.time()
    tr.fit(opts.max_steps, log_every=config.get("log_iter", 20))
    torch.cuda.synchronize()
    res = {"steps": tr.global_step, "seconds": time.time() - t0, "radii": tr.radii, "shuffle": tr.shuffle,
           "shuffle_seed": tr.shuffle_seed if tr.shuffle else None}
    res.update(tr.metrics())
    if image_dir is not None:
        last_epoch = max(0, -(-tr.global_step // tr.steps_per_epoch) - 1)
        stats = tr.save_validation_images(last_epoch, res, image_dir)
        if not tr._display_source()[1]:
            print(coil_stats_table(stats), flush=True)
    for i, sd in tr.checkpoints().items():
        torch.save(sd, os.path.join(ckpt_dir, "submodel_%d.pt" % i))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
