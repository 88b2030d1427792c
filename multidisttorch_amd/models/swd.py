"""Sliced Wasserstein distance between decoded prior samples and held-out
images. The oracle.

The sample report's other scores (models/sample_report.py, models/prdc.py) are
built on the pair matrix: O(N^2 D) work, and a scale set by a bandwidth or a k.
The sliced Wasserstein distance (Rabin et al. 2011; Karras et al. 2018; Kolouri
et al. 2019) is a metric on distributions in the units of the data: project
both sets on P random unit directions, take each projection's Wasserstein
distance between the two one-dimensional empirical measures (a closed form over
the sorted values) and average. Its standard error across the projections comes
with it, so it orders the trials of a sweep with an error bar, at O(P N D).

For ``real [na, D]``, ``fake [nb, D]`` and ``dirs [P, D]``::

    pr[p, i] = sum_c dirs[p, c] * real[i, c]        pf[p, j] likewise
    sr[p], sf[p] = pr[p], pf[p] sorted ascending
    # the two quantile functions on the common grid of na*nb cells: cell t holds sr[p, t // nb] and sf[p, t // na]
    w1[p]   = mean_t |sr[p, t // nb] - sf[p, t // na]|
    w2sq[p] = mean_t (sr[p, t // nb] - sf[p, t // na])^2

evaluated over the maximal runs of equal cells: the segments between consecutive
breakpoints of ``{i*nb} U {j*na}``, ``na + nb - gcd(na, nb)`` of them, each with
an integer length in units of ``1/(na*nb)``. For ``na == nb`` this is the usual
``mean_i |sr[i] - sf[i]|``.

The directions are Philox with the trial seed as key, stream word
``SWD_STREAM`` and step words 0 (``reparam_eps(P, D, seed, SWD_STREAM, 0)``),
normalised on the host: the result is a function of (weights, data, seed, n, P)
only.

Everything here is plain torch, dtype-generic (float64 for the tests' oracle);
the trainers' ``torch`` backends run it in float32, and the HIP kernels
(csrc/kernels/swd.hip) compute what ``swd_rows`` defines.
"""

from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from ..ops.philox import reparam_eps

__all__ = ["SWD_STREAM", "MAX_ROWS", "MAX_D", "MAX_DIRS", "COLS", "check_swd_args", "swd_directions", "swd_segments",
           "swd_rows", "swd_stats"]

SWD_STREAM = 6 << 28
MAX_ROWS = 16384  # per set: both sorted sets of one projection live in one workgroup's LDS
MAX_D = 65536
MAX_DIRS = 4096
COLS = 2  # a table row: w1, w2sq


def check_swd_args(na: int, nb: int, D: int, P: int):
    for name, n in (("real", na), ("generated", nb)):
        if int(n) != n or not 2 <= n <= MAX_ROWS:
            raise ValueError(f"the sliced Wasserstein distance supports 2 <= rows <= {MAX_ROWS} per set (both sorted "
                             f"sets of a projection are held in one workgroup's LDS), got {n!r} {name} rows")
    if int(D) != D or not 1 <= D <= MAX_D:
        raise ValueError(f"the sliced Wasserstein distance supports 1 <= D <= {MAX_D}, got D = {D!r}")
    if int(P) != P or not 1 <= P <= MAX_DIRS:
        raise ValueError(f"the sliced Wasserstein distance supports 1 <= directions <= {MAX_DIRS}, got {P!r}")


def swd_directions(P: int, D: int, seed: int) -> np.ndarray:
    """dirs[P, D] (float32): unit rows, normalised in float64."""
    g = reparam_eps(P, D, seed, SWD_STREAM, 0).astype(np.float64)
    norm = np.sqrt((g * g).sum(1, keepdims=True))
    if not bool((norm > 0).all()):
        raise ValueError("a sliced Wasserstein direction has zero length")
    return (g / norm).astype(np.float32)


def swd_segments(na: int, nb: int, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The maximal runs of equal cells of the common grid: ``(i, j, length)`` (int64), the real and fake order
    statistics a segment holds and its number of cells."""
    cuts = torch.unique(torch.cat([torch.arange(na + 1, device=device) * nb, torch.arange(nb + 1, device=device) * na]))
    start = cuts[:-1]
    return start // nb, start // na, cuts[1:] - start


def swd_rows(real: torch.Tensor, fake: torch.Tensor, dirs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(proj [P, na + nb], table [P, COLS])`` in the inputs' dtype: ``proj[p]`` is ``sr[p] | sf[p]``."""
    na, D = real.shape
    nb, P = fake.shape[0], dirs.shape[0]
    check_swd_args(na, nb, D, P)
    if fake.shape[1] != D or dirs.shape[1] != D:
        raise ValueError(f"real, generated rows and directions differ in width: {D}, {fake.shape[1]}, {dirs.shape[1]}")
    # products, then a sum: row by row of dirs, so that a block is [na + nb, D]
    U = torch.cat([real, fake])
    pu = torch.stack([(U * d[None]).sum(1) for d in dirs])
    sr, sf = pu[:, :na].sort(1).values, pu[:, na:].sort(1).values
    i, j, length = swd_segments(na, nb, real.device)
    diff = sr[:, i] - sf[:, j]
    w = length.to(real.dtype)[None] / float(na * nb)
    return torch.cat([sr, sf], 1), torch.stack([(diff.abs() * w).sum(1), (diff * diff * w).sum(1)], 1)


def swd_stats(table: torch.Tensor) -> Dict[str, object]:
    """The distance and its Monte-Carlo error from a per-direction table, in float64."""
    t = table.double()
    P = t.shape[0]
    w1 = t[:, 0]
    se = float(w1.std(unbiased=True)) / math.sqrt(P) if P > 1 else 0.0
    return dict(dirs=int(P), swd1=float(w1.mean()), swd1_se=se, swd2=math.sqrt(float(t[:, 1].mean())),
                max_w1=float(w1.max()))
