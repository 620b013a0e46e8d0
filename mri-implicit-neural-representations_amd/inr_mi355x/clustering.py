"""Ring partition of k-space by 1-D k-means (the reference's src/clustering.py:19-135), the preprocessing
that gives the multiscale loop its radii (train_kspace_multiscale.py:73-84).

The ring statistics run on whatever device holds the k-space: fp32 tensors on the GPU take all rings from one pass of the band
kernel (bands.band_stats, DESIGN.md 4.17: one call and one read-back per 64 rings); CPU tensors, and tensors of another
dtype, go through the reference's loop of masked reductions.  The k-means itself is 40 numbers and uses the same ``sklearn.cluster.KMeans(init="random", n_init=10,
max_iter=200, random_state=42)`` call as the reference, on the host.  Nothing is plotted.
"""
from math import sqrt
from typing import Tuple

import numpy as np
import torch


def _complex_abs(x: torch.Tensor) -> torch.Tensor:
    """fastmri.complex_abs: sqrt(re^2 + im^2) over the last axis (size 2)."""
    return torch.sqrt((x ** 2).sum(dim=-1))


def ring_bounds(no_steps: int):
    """clustering.py:48-57: ring i covers [sqrt2*i/n, sqrt2*(i+1)/n], both ends included."""
    out = []
    for i in range(no_steps):
        r0 = 0 if i == 0 else sqrt(2) * i / no_steps
        r1 = sqrt(2) if i == no_steps - 1 else sqrt(2) * (i + 1) / no_steps
        out.append((r0, r1))
    return out


def _on_kernel(img: torch.Tensor, dist: torch.Tensor) -> bool:
    """The band kernel reads fp32 device tensors; everything else keeps the loop of masked reductions."""
    return img.is_cuda and img.dtype == torch.float32 and dist.dtype == torch.float32


def _band_field_device(img: torch.Tensor, dist: torch.Tensor, bounds, field: str, what: str) -> np.ndarray:
    """``field`` of bands.band_stats per band, float32: one kernel call per 64 bands (the kernel's limit; the usual 40
    rings or 4 partitions are one call).  A band without a point raises, as the loop's max() of nothing does."""
    from . import _lib as L
    from .bands import band_stats
    d, g = dist.reshape(-1), img.reshape(-1, 2)
    out = []
    for k0 in range(0, len(bounds), L.BAND_MAX):
        st = band_stats(d, g, bounds=bounds[k0:k0 + L.BAND_MAX])
        for b in np.flatnonzero(st.n == 0):
            r0, r1 = bounds[k0 + b]
            raise RuntimeError(f"{what} {k0 + b} [{r0!r}, {r1!r}] of the partition holds no k-space point")
        out.append(getattr(st, field).astype(np.float32))
    return np.concatenate(out)


def _ring_logmax_device(img: torch.Tensor, dist: torch.Tensor, bounds) -> list:
    """max of log|z| per ring: sqrt and log are monotone, so the maximum of log(sqrt(re^2 + im^2)) is log(sqrt(.)) of
    the maximal fp32 re^2 + im^2 (max_abs2), evaluated here by the same CPU torch functions the loop below applies to
    every point of a CPU tensor."""
    return torch.log(torch.sqrt(torch.from_numpy(_band_field_device(img, dist, bounds, "max_abs2", "ring")))).tolist()


def _radius(kcoords: torch.Tensor) -> torch.Tensor:
    """dist_to_center of the reference: sqrt(ky^2 + kx^2) of (coil, y, x) coordinates"""
    return torch.sqrt(kcoords[..., 1] ** 2 + kcoords[..., 2] ** 2)


def partition_kspace(img: torch.Tensor, kcoords: torch.Tensor, no_steps: int = 40, no_parts: int = 4):
    """clustering.py:19-89.  img [C,H,W,2], kcoords [C,H,W,3] (coil, y, x).  Returns (labels of the no_steps
    initial rings, radii [no_parts+1] separating the final partitions; the last radius is 5 = 'everything')."""
    return partition_rows(img, _radius(kcoords), no_steps, no_parts)


def partition_rows(img: torch.Tensor, dist: torch.Tensor, no_steps: int = 40, no_parts: int = 4):
    """partition_kspace of rows: img [..., 2] with the radius ``dist`` [...] of every row (the grid's rows, or the
    off-grid samples of a trajectory with the radius of their own coordinates)."""
    from sklearn.cluster import KMeans
    if _on_kernel(img, dist):
        means = _ring_logmax_device(img, dist, ring_bounds(no_steps))
    else:
        logmag = torch.log(_complex_abs(img))
        means = []
        for r0, r1 in ring_bounds(no_steps):
            sel = (dist >= r0) & (dist <= r1)
            means.append(float(logmag[sel].max()))  # clustering.py:60-61 (named means, is the max)
    means = np.array(means).reshape(-1, 1)
    kmeans = KMeans(init="random", n_clusters=no_parts, n_init=10, max_iter=200, random_state=42)
    kmeans.fit(means)
    labels = kmeans.labels_
    # Walking outwards, every cluster claims as many of the initial rings as carry its label, in the order in which
    # the clusters are first met (clustering.py:72-84): boundary j = sqrt(2) * (rings claimed by the first j clusters)
    # / no_steps.  (Rings of one cluster are counted together even if another cluster's ring sits between them.)
    first_met, ring_count = [], {}
    for lab in labels.tolist():
        if lab not in ring_count:
            first_met.append(lab)
            ring_count[lab] = 0
        ring_count[lab] += 1
    claimed = np.cumsum([ring_count[lab] / len(labels) for lab in first_met])
    radii = np.concatenate(([0.0], sqrt(2) * claimed))
    radii[no_parts] = 5  # the outermost partition is "everything beyond" (clustering.py:82)
    return labels, radii


def partition_and_stats(img: torch.Tensor, kcoords: torch.Tensor, no_steps: int = 40, no_parts: int = 4,
                        stat: str = "max") -> Tuple[torch.Tensor, np.ndarray]:
    """clustering.py:91-135: per final partition the max (or min) of |component| of the k-space inside it."""
    return partition_and_stats_rows(img, _radius(kcoords), no_steps, no_parts, stat)


def partition_and_stats_rows(img: torch.Tensor, dist: torch.Tensor, no_steps: int = 40, no_parts: int = 4,
                             stat: str = "max") -> Tuple[torch.Tensor, np.ndarray]:
    """partition_and_stats of rows (see partition_rows); ring intervals are closed at both ends."""
    _, radii = partition_rows(img, dist, no_steps, no_parts)
    if _on_kernel(img, dist):
        bounds = [(float(radii[i]), float(radii[i + 1])) for i in range(len(radii) - 1)]
        vals = _band_field_device(img, dist, bounds, "min_comp" if stat == "min" else "max_comp", "partition")
        return torch.from_numpy(vals).to(img.device), radii
    stats = []
    for i in range(len(radii) - 1):
        sel = (dist >= radii[i]) & (dist <= radii[i + 1])
        a = torch.abs(img[sel])
        stats.append(a.min() if stat == "min" else a.max())
    return torch.stack(stats), radii
