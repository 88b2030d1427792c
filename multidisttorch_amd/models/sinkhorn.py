"""Debiased entropic optimal-transport distance (the Sinkhorn divergence) between
decoded prior samples and held-out images. The oracle.

The sample report's other scores have a scale set by a bandwidth or a k
(models/sample_report.py, models/prdc.py) or are distances between
one-dimensional shadows of the two sets (models/swd.py). The Sinkhorn divergence
(Genevay et al. 2018; Feydy et al. 2019) is the full-dimensional transport
distance ``S_eps = OT_eps(a, b) - OT_eps(a, a) / 2 - OT_eps(b, b) / 2``, in the
squared units of the data, and it comes with its own convergence measure.

For ``real [na, D]`` (x) and ``fake [nb, D]`` (y), uniform weights ``la = -log
na``, ``lb = -log nb`` and squared distances formed from differences::

    Cxy[i, j] = |x_i - y_j|^2      Cxx, Cyy likewise (their diagonals are exactly 0)
    m = mean_{i, j} Cxx[i, j]      over all na^2 entries
    eps_t = max(E, 4 * 0.5**t) * m                      t = 0 .. T-1
    softmin_row(C, h, lw, eps)[i] = -eps * logsumexp_j(lw + (h[j] - C[i, j]) / eps)

The potentials f [na], g [nb] (the pair), p [na], q [nb] (the two debiasing
problems) start at 0. Iterations ``t = 0 .. T-2`` are averaged and simultaneous::

    f' = (f + softmin_row(Cxy,   g, lb, eps_t)) / 2     g' = (g + softmin_row(Cxy^T, f, la, eps_t)) / 2
    p' = (p + softmin_row(Cxx,   p, la, eps_t)) / 2     q' = (q + softmin_row(Cyy,   q, lb, eps_t)) / 2

and the last, ``t = T-1``, replaces: ``ft = softmin_row(Cxy, g, lb, eps_{T-1})``
and ``gt``, ``pt``, ``qt`` likewise; ``marg[i] = |exp((f[i] - ft[i]) / eps_{T-1})
- 1|`` is the relative violation of row i's marginal by the plan that (f, g)
define. The fixed schedule makes the result a function of (rows, E, T) alone.

Everything here is plain torch, dtype-generic (float64 for the tests' oracle);
the trainers' ``torch`` backends run it in float32, and the HIP kernels
(csrc/kernels/sinkhorn.hip) compute what ``sinkhorn_rows`` defines.
"""

from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

__all__ = ["MAX_ROWS", "MAX_D", "MAX_BLUR", "MAX_ITERS", "COLS", "check_sinkhorn_args", "sinkhorn_costs", "sinkhorn_rows",
           "sinkhorn_stats"]

MAX_ROWS = 16384  # per set: the three cost matrices are stored, 3.2 GB of float32 at the cap
MAX_D = 65536
MAX_BLUR = 4.0    # the anneal starts at 4 m
MAX_ITERS = 10000
COLS = 2  # a table row: the pair's potential, the debiasing potential


def check_sinkhorn_args(na: int, nb: int, D: int, E: float, T: int):
    for name, n in (("real", na), ("generated", nb)):
        if int(n) != n or not 2 <= n <= MAX_ROWS:
            raise ValueError(f"the Sinkhorn divergence supports 2 <= rows <= {MAX_ROWS} per set (the cost matrices are "
                             f"stored), got {n!r} {name} rows")
    if int(D) != D or not 1 <= D <= MAX_D:
        raise ValueError(f"the Sinkhorn divergence supports 1 <= D <= {MAX_D}, got D = {D!r}")
    if not (isinstance(E, (int, float)) and math.isfinite(E) and 0 < E <= MAX_BLUR):
        raise ValueError(f"the Sinkhorn blur is a fraction 0 < E <= {MAX_BLUR:g} of the mean squared distance, got {E!r}")
    if int(T) != T or not 1 <= T <= MAX_ITERS:
        raise ValueError(f"the Sinkhorn divergence supports 1 <= iterations <= {MAX_ITERS}, got {T!r}")


def _sqdist(x: torch.Tensor, y: torch.Tensor, block_elems: int = 1 << 22) -> torch.Tensor:
    """[n, m] squared distances from differences, in row blocks of about ``block_elems`` differences."""
    step = max(1, block_elems // max(1, y.shape[0] * y.shape[1]))
    return torch.cat([((x[i: i + step, None, :] - y[None]) ** 2).sum(2) for i in range(0, x.shape[0], step)])


def sinkhorn_costs(real: torch.Tensor, fake: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(Cxy [na, nb], Cxx [na, na], Cyy [nb, nb], m)`` in the inputs' dtype."""
    Cxx = _sqdist(real, real)
    return _sqdist(real, fake), Cxx, _sqdist(fake, fake), Cxx.mean()


def softmin_row(C: torch.Tensor, h: torch.Tensor, lw: float, eps) -> torch.Tensor:
    return -eps * torch.logsumexp(lw + (h[None, :] - C) / eps, dim=1)


def sinkhorn_rows(real: torch.Tensor, fake: torch.Tensor, E: float, T: int, costs=None):
    """``(pot [na + nb, COLS], m, marg_err)`` in the inputs' dtype: ``pot[:, 0]`` is ``ft | gt``, ``pot[:, 1]``
    is ``pt | qt``; ``m`` and ``marg_err`` are 0-d tensors. ``costs``: a ``sinkhorn_costs`` result of the same rows."""
    na, D = real.shape
    nb = fake.shape[0]
    check_sinkhorn_args(na, nb, D, E, T)
    if fake.shape[1] != D:
        raise ValueError(f"real and generated rows differ in width: {D}, {fake.shape[1]}")
    Cxy, Cxx, Cyy, m = sinkhorn_costs(real, fake) if costs is None else costs
    Cyx = Cxy.t()
    la, lb = -math.log(na), -math.log(nb)
    f, p = (torch.zeros(na, dtype=real.dtype, device=real.device) for _ in range(2))
    g, q = (torch.zeros(nb, dtype=real.dtype, device=real.device) for _ in range(2))
    for t in range(T):
        eps = max(float(E), 4.0 * 0.5 ** t) * m
        ft, gt = softmin_row(Cxy, g, lb, eps), softmin_row(Cyx, f, la, eps)
        pt, qt = softmin_row(Cxx, p, la, eps), softmin_row(Cyy, q, lb, eps)
        if t < T - 1:
            f, g, p, q = (f + ft) / 2, (g + gt) / 2, (p + pt) / 2, (q + qt) / 2
    marg = (torch.exp((f - ft) / eps) - 1).abs()
    return torch.stack([torch.cat([ft, gt]), torch.cat([pt, qt])], 1), m, marg.mean()


def sinkhorn_stats(pot: torch.Tensor, na: int, m, marg_err, E: float, T: int) -> Dict[str, object]:
    """The distance from the potentials' table, on the host in float64."""
    m = float(m)
    if not m > 0.0:
        raise ValueError("the Sinkhorn blur is a fraction of the mean squared distance of the real rows, which is 0: "
                         "all real rows are equal")
    t = pot.double()
    f, g = t[:na], t[na:]
    s = float((f[:, 0] - f[:, 1]).mean() + (g[:, 0] - g[:, 1]).mean())
    return dict(blur=float(E), iters=int(T), scale=m, sinkhorn=s, w2=math.sqrt(max(s, 0.0)),
                ot=float(f[:, 0].mean() + g[:, 0].mean()), marg_err=float(marg_err))
