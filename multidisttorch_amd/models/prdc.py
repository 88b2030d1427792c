"""Precision, recall, density and coverage of decoded prior samples against
held-out images, on k-nearest-neighbour radii in pixel space. The oracle.

The sample report's two scores (models/sample_report.py) are single numbers:
when a sweep moves them they cannot say whether the samples left the data
manifold (fidelity) or stopped covering it (diversity). The k-NN manifold
estimate separates the two: improved precision and recall (Kynkaanniemi et al.
2019) and their outlier-robust form, density and coverage (Naeem et al. 2020).

For ``real [na, D]``, ``fake [nb, D]``, an integer k and
``d2(a, b) = sum_c (a_c - b_c)^2``::

    rad[i]   = the k-th smallest d2(row i, row j) over j != i in row i's own set,
               counting multiplicity (the k-th order statistic)
    cnt[j]   for a fake row j: #{ real i : d2(i, j) <= rad[i] }
    cnt[i]   for a real row i: #{ fake j : d2(i, j) <= rad[j] }
    dminx[i] = min over the other set of d2

    precision = share of fake rows with cnt > 0       recall   = share of real rows with cnt > 0
    density   = sum over fake rows of cnt / (k nb)    coverage = share of real rows with dminx[i] <= rad[i]

Everything here is plain torch, dtype-generic (float64 for the tests' oracle).
Distances come from differences, never from a Gram product; the trainers'
``torch`` backends run this in float32, chunked over i, and the HIP kernels
(csrc/kernels/prdc.hip) compute the per-row table ``prdc_rows`` defines.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

__all__ = ["MAX_K", "MAX_ROWS", "MAX_D", "COLS", "check_prdc_args", "prdc_rows", "prdc_stats"]

MAX_K = 8
MAX_ROWS = 32768  # per set
MAX_D = 65536
COLS = 3  # a table row: rad, cnt, dminx


def check_prdc_args(na: int, nb: int, D: int, k: int):
    if int(k) != k or not 1 <= k <= MAX_K:
        raise ValueError(f"PRDC supports 1 <= k <= {MAX_K}, got k = {k!r}")
    for name, n in (("real", na), ("generated", nb)):
        if int(n) != n or not k + 1 <= n <= MAX_ROWS:
            raise ValueError(f"PRDC at k = {k} supports {k + 1} <= rows <= {MAX_ROWS} per set (every row needs k "
                             f"other rows of its own set), got {n!r} {name} rows")
    if int(D) != D or not 1 <= D <= MAX_D:
        raise ValueError(f"PRDC supports 1 <= D <= {MAX_D}, got D = {D!r}")


def _pair_d2(A: torch.Tensor, B: torch.Tensor, step: int):
    """Blocks ``(i0, d2 [c, len(B)])`` of the pair distances of A's rows to B's, from differences."""
    for i0 in range(0, A.shape[0], step):
        yield i0, ((A[i0: i0 + step, None, :] - B[None]) ** 2).sum(-1)


def _radii(X: torch.Tensor, k: int, step: int) -> torch.Tensor:
    inf = torch.tensor(float("inf"), dtype=X.dtype, device=X.device)
    cols = torch.arange(X.shape[0], device=X.device)
    out = []
    for i0, d2 in _pair_d2(X, X, step):
        self_ = cols[None] == (i0 + torch.arange(d2.shape[0], device=X.device))[:, None]
        out.append(torch.where(self_, inf, d2).kthvalue(k, dim=1).values)
    return torch.cat(out)


def prdc_rows(real: torch.Tensor, fake: torch.Tensor, k: int, chunk: Optional[int] = None) -> torch.Tensor:
    """The per-row table ``[na + nb, COLS]`` in the inputs' dtype. ``chunk``:
    rows i per ``[chunk, rows of the other operand, D]`` block (default: all at once)."""
    na, D = real.shape
    nb = fake.shape[0]
    check_prdc_args(na, nb, D, k)
    if fake.shape[1] != D:
        raise ValueError(f"real and generated rows differ in width: {D} and {fake.shape[1]}")
    step = max(na, nb) if chunk is None else max(1, int(chunk))
    rad_r, rad_f = _radii(real, k, step), _radii(fake, k, step)
    cnt_f = torch.zeros(nb, dtype=real.dtype, device=real.device)
    dmin_f = torch.full((nb,), float("inf"), dtype=real.dtype, device=real.device)
    cnt_r, dmin_r = [], []
    for i0, d2 in _pair_d2(real, fake, step):  # [c, nb]: each cross block serves both ways
        cnt_r.append((d2 <= rad_f[None]).sum(1).to(real.dtype))
        dmin_r.append(d2.min(1).values)
        cnt_f += (d2 <= rad_r[i0: i0 + d2.shape[0], None]).sum(0).to(real.dtype)
        dmin_f = torch.minimum(dmin_f, d2.min(0).values)
    return torch.stack([torch.cat([rad_r, rad_f]), torch.cat(cnt_r + [cnt_f]), torch.cat(dmin_r + [dmin_f])], 1)


def prdc_stats(table: torch.Tensor, na: int, nb: int, k: int) -> Dict[str, object]:
    """The four numbers of a per-row table, in float64."""
    t = table.double()
    r, f = t[:na], t[na:]
    return dict(k=int(k), precision=float((f[:, 1] > 0).double().mean()), recall=float((r[:, 1] > 0).double().mean()),
                density=float(f[:, 1].sum()) / (k * nb), coverage=float((r[:, 2] <= r[:, 0]).double().mean()))
