"""Mode coverage of decoded prior samples: NDB, the number of statistically
different bins, and the Jensen-Shannon divergence of the bin histograms, on
k-means cells of the held-out images in pixel space. The oracle.

The sample report's other scores compare the two sets as wholes
(models/sample_report.py, prdc.py, swd.py, sinkhorn.py). NDB (Richardson & Weiss
2018) asks which kinds of image are missing: the real rows are clustered into K
Voronoi cells, both sets are counted per cell, and a cell is "different" when a
pooled two-proportion z-test rejects equal shares at ``|z| > 1.96``.

For ``real [na, D]`` (x), ``fake [nb, D]``, K cells, T Lloyd iterations and
``init_idx [K]`` (distinct real-row indices; ``ndb_init_idx`` draws them from a
seeded host permutation, so no floating-point decision picks them)::

    c_k = x[init_idx[k]]
    t = 0 .. T-1:   label[i] = argmin_k |x_i - c_k|^2      from differences, ties to the lowest k
                    c_k = mean of its rows                 a cell with no rows keeps c_k bit for bit
                    moved_t = #{i: label changed}          na at t = 0
    labels, mind = one more assignment of real | fake to the final centroids
    inertia = sum(mind[:na])

There is no early stop: the result is a function of (rows, K, T, init_idx) alone.

Everything here is plain torch, dtype-generic (float64 for the tests' oracle);
the trainers' ``torch`` backends run it in float32, and the HIP kernels
(csrc/kernels/kmeans.hip) compute what ``kmeans_rows`` defines.
"""

from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

__all__ = ["MAX_K", "MAX_ROWS", "MAX_D", "MAX_ITERS", "Z_CRIT", "check_ndb_args", "ndb_init_idx", "kmeans_assign",
           "kmeans_update", "kmeans_rows", "ndb_stats"]

MAX_K = 256       # the assignment keeps a band's scores against every centroid in registers
MAX_ROWS = 65536  # per set
MAX_D = 65536
MAX_ITERS = 1000
Z_CRIT = 1.96     # two-sided 5 %


def check_ndb_args(na: int, nb: int, D: int, K: int, T: int):
    for name, n in (("real", na), ("generated", nb)):
        if int(n) != n or not 2 <= n <= MAX_ROWS:
            raise ValueError(f"NDB supports 2 <= rows <= {MAX_ROWS} per set, got {n!r} {name} rows")
    if int(D) != D or not 1 <= D <= MAX_D:
        raise ValueError(f"NDB supports 1 <= D <= {MAX_D}, got D = {D!r}")
    if int(K) != K or not 2 <= K <= MAX_K:
        raise ValueError(f"NDB supports 2 <= K <= {MAX_K} bins, got K = {K!r}")
    if K > na:
        raise ValueError(f"NDB starts its K bins from distinct real rows: K = {K!r} needs at least as many, got {na!r}")
    if int(T) != T or not 1 <= T <= MAX_ITERS:
        raise ValueError(f"NDB supports 1 <= k-means iterations <= {MAX_ITERS}, got {T!r}")


def ndb_init_idx(na: int, K: int, seed: int, group_id: int = 0) -> torch.Tensor:
    """K distinct row indices (int64, on the host) from the run seed and the trial's group id."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(group_id) * 7919 + 0x4E4442) & 0x7FFFFFFFFFFFFFFF)
    return torch.randperm(int(na), generator=g)[: int(K)].contiguous()


def kmeans_assign(x: torch.Tensor, cent: torch.Tensor, block_elems: int = 1 << 22) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(label [n] int64, mind [n])``: the nearest centroid from differences, ties to the lowest k."""
    step = max(1, block_elems // max(1, cent.shape[0] * cent.shape[1]))
    d = torch.cat([((x[i: i + step, None, :] - cent[None]) ** 2).sum(2) for i in range(0, x.shape[0], step)])
    mind = d.min(1).values
    K = cent.shape[0]
    ks = torch.arange(K, device=x.device)
    return torch.where(d == mind[:, None], ks[None], K).min(1).values, mind


def kmeans_update(x: torch.Tensor, label: torch.Tensor, cent: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(centroids [K, D], counts [K] int64)``: the mean of each cell's rows; an empty cell keeps its centroid."""
    K = cent.shape[0]
    cnt = torch.bincount(label, minlength=K)
    s = torch.zeros_like(cent).index_add_(0, label, x)
    return torch.where((cnt > 0)[:, None], s / cnt.clamp(min=1).to(x.dtype)[:, None], cent), cnt


def kmeans_rows(real: torch.Tensor, fake: torch.Tensor, K: int, T: int, init_idx: torch.Tensor):
    """``(labels [na + nb] int64, mind [na + nb], centroids [K, D], moved [T] int64, inertia)`` in the inputs'
    dtype; ``inertia`` is a 0-d tensor."""
    na, D = real.shape
    nb = fake.shape[0]
    check_ndb_args(na, nb, D, K, T)
    if fake.shape[1] != D:
        raise ValueError(f"real and generated rows differ in width: {D}, {fake.shape[1]}")
    init_idx = init_idx.to(device=real.device, dtype=torch.int64)
    if init_idx.shape != (K,) or init_idx.unique().numel() != K or int(init_idx.min()) < 0 or int(init_idx.max()) >= na:
        raise ValueError(f"init_idx must hold K = {K} distinct real-row indices")
    cent = real[init_idx].clone()
    label = torch.full((na,), -1, dtype=torch.int64, device=real.device)
    moved = []
    for _ in range(T):
        new, _ = kmeans_assign(real, cent)
        moved.append((new != label).sum())
        label = new
        cent, _ = kmeans_update(real, label, cent)
    labels, mind = kmeans_assign(torch.cat([real, fake]), cent)
    return labels, mind, cent, torch.stack(moved), mind[:na].sum()


def ndb_stats(labels: torch.Tensor, na: int, K: int, inertia=0.0, moved=0, T: int = 0) -> Dict[str, object]:
    """The bins' statistics from the labels of real | generated rows, on the host in float64 and integers."""
    lab = labels.to("cpu", torch.int64)
    nb = lab.numel() - na
    cr = torch.bincount(lab[:na], minlength=K).tolist()
    cf = torch.bincount(lab[na:], minlength=K).tolist()
    ndb, jsd = 0, 0.0
    for r, f in zip(cr, cf):
        p, q = r / na, f / nb
        pool = (r + f) / (na + nb)
        se = math.sqrt(pool * (1.0 - pool) * (1.0 / na + 1.0 / nb))
        if r + f > 0 and se > 0.0 and abs(p - q) / se > Z_CRIT:
            ndb += 1
        mid = 0.5 * (p + q)
        jsd += (0.5 * p * math.log(p / mid) if p > 0 else 0.0) + (0.5 * q * math.log(q / mid) if q > 0 else 0.0)
    return dict(K=int(K), iters=int(T), ndb=ndb, ndb_over_k=ndb / K, jsd=max(jsd, 0.0),
                missing=sum(1 for r, f in zip(cr, cf) if r > 0 and f == 0), inertia=float(inertia), moved=int(moved),
                counts_real=cr, counts_fake=cf)
