"""Sample report of a VAE: kernel MMD and the 1-NN two-sample test between
decoded prior samples and held-out images. The oracle.

What the decoder produces from the prior, scored without a pretrained network
(the two sample-based scores of Xu et al. 2018 that work in pixel space): the
unbiased kernel maximum mean discrepancy (Gretton et al. 2012) and the
leave-one-out accuracy of a 1-nearest-neighbour classifier on the union
(Lopez-Paz & Oquab 2017), 0.5 being ideal; a high generated half with a low real
half means blur or mode collapse, the opposite memorisation.

For ``real [na, D]`` and ``fake [nb, D]`` with the union U = real rows | fake
rows, and all sums and minima over j != i::

    d2[i,j]   = sum_k (U[i,k] - U[j,k])^2
    m         = 2 na/(na-1) * sum_k Var_i(real[i,k])     # population variance: the mean of d2 over real pairs i != j
    h_s       = c_s * m,  c = BANDWIDTH_SCALES            # from the real rows only: one kernel per run
    k_s(i,j)  = exp(-d2[i,j] / h_s)
    dmin_r[i] = min_{j real} d2     dmin_f[i] = min_{j fake} d2
    ksum_r[i,s] = sum_{j real} k_s  ksum_f[i,s] = sum_{j fake} k_s
    RR = sum_{i real} ksum_r   FF = sum_{i fake} ksum_f   RF = sum_{i real} ksum_f   FR = sum_{i fake} ksum_r
    mmd2_s = RR/(na(na-1)) + FF/(nb(nb-1)) - 2 RF/(na nb)      mmd2 = mean_s mmd2_s
    rf_asym = |RF - FR| / RF                                     # the cross term both ways: a self-check
    neighbour of i is real iff dmin_r[i] <= dmin_f[i]            # a tie counts as real
    nn_acc_real = share of real rows with a real neighbour       nn_acc_fake = share of fake rows with a fake one
    nn_acc = share of all rows that are right
    nn_dist_real_to_fake = mean_{i real} sqrt(dmin_f)  (coverage)   nn_dist_fake_to_real = mean_{i fake} sqrt(dmin_r)  (fidelity)

The mean of the three Gaussians is itself a kernel, so ``mmd2`` is an MMD.

The pass's z is Philox with the trial seed as key, stream word
``SAMPLE_STREAM``, step words 0 and counter ``i*Z + c``
(``reparam_eps(n, Z, seed, SAMPLE_STREAM, 0)``), formed on the host:
``rng_stream`` does not enter and the result is a function of (weights, data,
seed, n) only.

Everything here is plain torch, dtype-generic (float64 for the tests' oracle).
Distances come from differences, never from a Gram product; the trainers'
``torch`` backends run this in float32, chunked over i, and the HIP kernels
(csrc/kernels/two_sample.hip) compute the per-row table ``sample_rows`` defines.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ..ops.philox import reparam_eps

__all__ = ["SAMPLE_STREAM", "BANDWIDTH_SCALES", "MAX_ROWS", "MAX_D", "COLS", "check_sample_args", "sample_z",
           "mean_pair_d2", "bandwidths_of", "sample_rows", "sample_stats", "sample_report"]

SAMPLE_STREAM = 5 << 28
BANDWIDTH_SCALES = (0.25, 1.0, 4.0)
MAX_ROWS = 32768  # per set: the union's row index and the strip partials stay small
MAX_D = 65536
COLS = 2 + 2 * len(BANDWIDTH_SCALES)  # a table row: dmin_r, dmin_f, ksum_r[3], ksum_f[3]


def check_sample_args(na: int, nb: int, D: int):
    for name, n in (("real", na), ("generated", nb)):
        if int(n) != n or not 2 <= n <= MAX_ROWS:
            raise ValueError(f"the sample report supports 2 <= rows <= {MAX_ROWS} per set, got {n!r} {name} rows")
    if int(D) != D or not 1 <= D <= MAX_D:
        raise ValueError(f"the sample report supports 1 <= D <= {MAX_D}, got D = {D!r}")


def sample_z(n: int, Z: int, seed: int) -> np.ndarray:
    """z[n, Z] (float32) of a pass over n samples."""
    return reparam_eps(n, Z, seed, SAMPLE_STREAM, 0)


def mean_pair_d2(real: torch.Tensor) -> float:
    """m: the mean of d2 over the real pairs i != j, in closed form in float64."""
    na = real.shape[0]
    m = 2.0 * na / (na - 1) * float(real.double().var(0, unbiased=False).sum())
    if not m > 0.0:
        raise ValueError("the sample report needs real rows that differ: their mean pair distance is 0")
    return m


def bandwidths_of(m: float) -> tuple:
    return tuple(c * m for c in BANDWIDTH_SCALES)


def sample_rows(real: torch.Tensor, fake: torch.Tensor, bandwidths: Sequence[float],
                chunk: Optional[int] = None) -> torch.Tensor:
    """The per-row table ``[na + nb, COLS]`` in the inputs' dtype. ``chunk``:
    rows i per ``[chunk, na + nb, D]`` block (default: all at once)."""
    na, D = real.shape
    nb = fake.shape[0]
    check_sample_args(na, nb, D)
    if fake.shape[1] != D:
        raise ValueError(f"real and generated rows differ in width: {D} and {fake.shape[1]}")
    U = torch.cat([real, fake])
    N = na + nb
    step = N if chunk is None else max(1, int(chunk))
    inf = torch.tensor(float("inf"), dtype=U.dtype, device=U.device)
    cols = torch.arange(N, device=U.device)
    out = []
    for i0 in range(0, N, step):
        Ui = U[i0: i0 + step]
        d2 = ((Ui[:, None, :] - U[None]) ** 2).sum(-1)                      # [c, N]
        self_ = cols[None] == (i0 + torch.arange(Ui.shape[0], device=U.device))[:, None]
        dm = torch.where(self_, inf, d2)
        row = [dm[:, :na].min(1).values, dm[:, na:].min(1).values]
        ks = [torch.where(self_, torch.zeros_like(d2), torch.exp(-d2 / h)) for h in bandwidths]
        row += [k[:, :na].sum(1) for k in ks] + [k[:, na:].sum(1) for k in ks]
        out.append(torch.stack(row, 1))
    return torch.cat(out)


def sample_stats(table: torch.Tensor, na: int, nb: int) -> Dict[str, object]:
    """MMD, accuracies and mean neighbour distances of a per-row table, in float64."""
    S = len(BANDWIDTH_SCALES)
    t = table.double()
    r, f = t[:na], t[na:]
    RR, RF = r[:, 2:2 + S].sum(0), r[:, 2 + S:].sum(0)
    FR, FF = f[:, 2:2 + S].sum(0), f[:, 2 + S:].sum(0)
    per = RR / (na * (na - 1)) + FF / (nb * (nb - 1)) - 2.0 * RF / (na * nb)
    real_right = int((r[:, 0] <= r[:, 1]).sum())
    fake_right = int((f[:, 0] > f[:, 1]).sum())
    return dict(mmd2=float(per.mean()), mmd2_per_bandwidth=[float(v) for v in per],
                nn_acc=(real_right + fake_right) / (na + nb), nn_acc_real=real_right / na, nn_acc_fake=fake_right / nb,
                nn_dist_real_to_fake=float(r[:, 1].sqrt().mean()), nn_dist_fake_to_real=float(f[:, 0].sqrt().mean()),
                rf_asym=float(((RF - FR).abs() / RF).max()))


def sample_report(real: torch.Tensor, fake: torch.Tensor, bandwidths: Optional[Sequence[float]] = None,
                  chunk: Optional[int] = None, return_rows: bool = False) -> Dict[str, object]:
    """The report of ``real [na, D]`` against ``fake [nb, D]`` in their dtype.
    ``bandwidths``: the three h_s (default: from the real rows)."""
    na, D = real.shape
    nb = fake.shape[0]
    check_sample_args(na, nb, D)
    m = mean_pair_d2(real)
    h = bandwidths_of(m) if bandwidths is None else tuple(float(v) for v in bandwidths)
    table = sample_rows(real, fake, h, chunk)
    out = dict(rows_real=int(na), rows_fake=int(nb), mean_pair_d2=m, bandwidths=list(h), **sample_stats(table, na, nb))
    if return_rows:
        out["table"] = table
    return out
