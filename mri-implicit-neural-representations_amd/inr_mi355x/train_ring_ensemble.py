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

from typing import List, Optional, Sequence

import numpy as np
import torch

from .cli import cli_band_report, cli_data, cli_fit_data, cli_folders, cli_validation_images, parse_cli, print_band_tables
from .engine import LossSpec
from .train import MODELS, MFN_MODELS
from .trainer_base import ResidentFit, mlp_engine


def ring_owner(i: int, world: int) -> int:
    return i % world


def winning_ring(dist: torch.Tensor, radii: Sequence[float]) -> torch.Tensor:
    """Index of the LAST ring containing each point (-1: none), i.e. the one whose output survives the
    sequential overwrite of train_clustering.py:199-211."""
    win = torch.full(dist.shape, -1, dtype=torch.int64, device=dist.device)
    for i in range(len(radii) - 1):
        win[(dist >= radii[i]) & (dist <= radii[i + 1])] = i
    return win


class RingEnsembleTrainer(ResidentFit):
    predict_chunk = 1 << 17

    def __init__(self, config: dict, image: torch.Tensor, coords: torch.Tensor, shape, device,
                 radii: Optional[Sequence[float]] = None, seed: int = 0, rank: int = 0, world: int = 1,
                 process_group=None, jitter: float = 0.0, coil_compression=None):
        config = self._init_fit(config, shape, device, seed, rank, world, process_group,
                                coil_compression=coil_compression)
        self.in_image_space = bool(config.get("transform", False))
        if config.get("loss") == "FFL":  # its weight is relative to the batch's largest error: a ring sees only its rows
            raise NotImplementedError("loss 'FFL' (focal frequency loss): ring ensembles train through the fused step; "
                                      "FFL fits run in INRTrainer (python -m inr_mi355x.train) only")
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
        self._seeded_encoder(seed)
        # (a rank may own no ring and still encodes its batches: enc_B does not wait for an engine)
        self.enc_B = self.encoder.B.contiguous() if config["encoder"]["embedding"] == "gauss" else None
        self.models, self.engines = {}, {}
        for i in range(self.no_models):
            m = MODELS[config["model"]](config["net"])
            if i in self.owned:
                m = m.to(self.device)
                self.models[i] = m
                self.engines[i] = mlp_engine(m, self.encoder, config["encoder"])[0]
        self.loss = LossSpec.from_config(config)
        # no mask and plain batches (image_full is the image itself); in a shuffled fit every rank fills its own epoch
        # buffers with the same order, and dist is recomputed from the epoch's coordinates (_refilled)
        self._resident_data(image, coords)
        self._init_validation()
        self.dist = self._t_dist = torch.sqrt(self.coords[:, 1] ** 2 + self.coords[:, 2] ** 2)
        self.jitter = float(jitter)
        self._rng = np.random.RandomState(seed)
        self._masks = {}

    def _default_band_bounds(self):
        """the ensemble's own rings"""
        return [(self.radii[i], self.radii[i + 1]) for i in range(self.no_models)]

    def _batch_hdr_A(self, it: int, lo: int, hi: int) -> float:
        return 0.0  # loss 'HDR' is not refused here, and the ring loop has never handed the kernels an A

    def _refilled(self) -> None:
        """Every ring's row mask over the whole epoch buffer and its per-batch counts -- one batched op and one read-back
        (the cached masks are tied to the batches' contents)."""
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
                lo, hi = self._range(b)
                self._masks[(i, lo)] = (masks[i, lo:hi], counts[i][b])

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
            it = self._begin_shuffled(epoch, it)
        lo, hi = self._range(it)
        lr = self._lr(epoch)
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

    def _log_value(self, losses):
        return [None if l is None else float(l) for l in losses]

    def _forward_chunk(self, lo: int, hi: int) -> torch.Tensor:
        """Each point from the last ring that contains it (train_clustering.py:199-211); zeros where that ring is
        another rank's."""
        rec = torch.zeros(hi - lo, 2, device=self.device)
        win = winning_ring(self.dist[lo:hi], self.radii)
        x = self._inputs(lo, hi)
        for i in self.owned:
            sel = win == i
            if bool(sel.any()):
                rec[sel] = self.engines[i].forward(x, self.enc_B, save=False)[sel]
        return rec

    @torch.no_grad()
    def predict_all(self, chunk: Optional[int] = None) -> torch.Tensor:
        """[N,2] reconstruction: ranks contribute their rings' rows and one SUM all-reduce assembles the whole.  (metrics()
        has no test loss: the reference's ring loop has no validation epoch.  Every rank that calls it after this
        all-reduce gets the same numbers.)"""
        rec = super().predict_all(chunk)
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=self.pg)
        return rec

    def checkpoints(self) -> dict:
        """{ring: {'net', 'enc'}} of the owned rings (submodel_%d files of train_clustering.py:243-249)."""
        out = {i: {"net": self.models[i].state_dict(), "enc": self.encoder.B} for i in self.owned}
        if self.coil_compression is not None:
            for sd in out.values():
                sd["coil_compression"] = self.coil_compression.state()
        return out


def main():
    """python -m inr_mi355x.train_ring_ensemble --config cfg.yaml [--output_path out] [--synthetic C,H,W]
    [--max_steps N] [--shuffle] [--shuffle-seed S] [--save-images] [--band-report [N]] [--virtual-coils K]: fit the rings (radii from
    config['partition']), print
    one JSON line with the assembled reconstruction's PSNR / SSIM and save the submodel_%d files of
    train_clustering.py:243-249.  --save-images writes train.png / train_kspace.png and the final metrics()' pictures
    to <output_path>/images (the ring loop has no validation epoch), the submodels to <output_path>/checkpoints, and
    prints the per-coil table.  --band-report prints the final metrics()' error by radius (per ring of the ensemble, or N
    rings) and adds it to the JSON line as 'bands'."""
    import json
    import os
    import time

    opts, config = parse_cli(val_and_samples=False)
    image, coords, shape, cc = cli_fit_data(opts, config, "coil", image_space=bool(config.get("transform", False)))
    tr = RingEnsembleTrainer(config, image, coords, shape, "cuda", coil_compression=cc)
    ckpt_dir, image_dir = cli_folders(tr, opts)
    cli_band_report(tr, opts)
    t0 = time.time()
    tr.fit(opts.max_steps, log_every=config.get("log_iter", 20))
    torch.cuda.synchronize()
    res = {"steps": tr.global_step, "seconds": time.time() - t0, "radii": tr.radii, "shuffle": tr.shuffle,
           "shuffle_seed": tr.shuffle_seed if tr.shuffle else None}
    res.update(tr.metrics())
    print_band_tables(res)
    if image_dir is not None:
        last_epoch = max(0, -(-tr.global_step // tr.steps_per_epoch) - 1)
        cli_validation_images(tr, last_epoch, res, image_dir)
    for i, sd in tr.checkpoints().items():
        torch.save(sd, os.path.join(ckpt_dir, "submodel_%d.pt" % i))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
