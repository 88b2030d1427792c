"""Latent report of a VAE over a set of rows: active units and the MI / TC /
dimension-wise-KL split of the KL term. The oracle.

Why a trial of a beta sweep scored as it did: how many latent dimensions are
alive (Burda et al.: dimension d is active when ``Var_x(mu_d(x)) > 0.01``), and
how ``E_x KL(q(z|x) || p(z))`` splits into index-code mutual information
``I(x; z)``, total correlation ``TC(z)`` and dimension-wise KL (Hoffman &
Johnson; Chen et al., beta-TCVAE) -- the three terms beta acts on.

For rows i = 0..n-1 with encoder outputs ``mu, lv [n, Z]`` and one draw
``eps [n, Z]``::

    z        = mu + eps * exp(lv / 2)
    t[i,j,d] = -0.5 * ((z[i,d] - mu[j,d])^2 * exp(-lv[j,d]) + lv[j,d] + log(2 pi))    # log q(z_id | x_j)
    lq_cond[i]  = sum_d t[i,i,d]
    lq_joint[i] = logsumexp_j( sum_d t[i,j,d] ) - log n
    lq_marg[i]  = sum_d ( logsumexp_j t[i,j,d] - log n )
    lp[i]       = sum_d -0.5 * (z[i,d]^2 + log(2 pi))
    mi   = mean_i(lq_cond - lq_joint)    tc = mean_i(lq_joint - lq_marg)    dwkl = mean_i(lq_marg - lp)
    sampled_kl = mean_i(lq_cond - lp)    # == mi + tc + dwkl, identically
    kl_per_dim[d] = mean_i 0.5*(mu^2 + exp(lv) - lv - 1)    kl = sum_d kl_per_dim
    mu_var[d]  = population variance over i of mu[i,d]      post_var[d] = mean_i exp(lv[i,d])
    active_units = #{d : mu_var[d] > au_threshold}

The aggregate posterior is that of the evaluated rows themselves (the full-set
form of Chen et al.'s estimator), so ``mi <= log n``. All outputs are per-row
means in nats.

The noise is Philox with the trial seed as key, stream word ``LATENT_STREAM``,
step words 0 and counter ``i*Z + c`` with i the row's position in the pass
(``reparam_eps(n, Z, seed, LATENT_STREAM, 0)``). ``rng_stream`` does not enter:
every replica of a group computes the same numbers, and the result is a pure
function of (weights, data, seed, n) -- not of the batch size, beta or the
schedules.

Everything here is plain torch, dtype-generic (float64 for the tests' oracle);
the trainers' ``torch`` backends run it in float32, chunked over i so that the
``[n, n, Z]`` tensor never exists, and the HIP kernels
(csrc/kernels/vae_latent.hip) implement it.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from ..ops.philox import reparam_eps

__all__ = ["LATENT_STREAM", "MAX_Z", "check_latent_args", "latent_eps", "latent_report"]

LATENT_STREAM = 3 << 28
MAX_Z = 64  # the HIP pair kernel keeps a row's Z accumulator pairs in registers
LOG_2PI = math.log(2.0 * math.pi)


def check_latent_args(n: int, Z: int, au_threshold: float = 0.01):
    if int(n) != n or n < 1:
        raise ValueError(f"the latent report needs at least one row, got n = {n!r}")
    if int(Z) != Z or not 1 <= Z <= MAX_Z:
        raise ValueError(f"the latent report supports 1 <= Z <= {MAX_Z}, got Z = {Z!r}")
    if n * Z > 2 ** 32:
        raise ValueError(f"n*Z = {n * Z} exceeds the 2^32 Philox counter range of one pass")
    if not (au_threshold >= 0.0):
        raise ValueError(f"au_threshold must be >= 0, got {au_threshold!r}")


def latent_eps(n: int, Z: int, seed: int) -> np.ndarray:
    """eps[n, Z] (float32) of a pass over n rows, as the kernels draw it."""
    return reparam_eps(n, Z, seed, LATENT_STREAM, 0)


def latent_report(mu: torch.Tensor, lv: torch.Tensor, eps: torch.Tensor, au_threshold: float = 0.01,
                  chunk: Optional[int] = None, return_rows: bool = False) -> Dict[str, object]:
    """The report of ``mu, lv, eps [n, Z]`` in their dtype. ``chunk``: rows i
    per ``[chunk, n, Z]`` block (default: all at once)."""
    n, Z = mu.shape
    check_latent_args(n, Z, au_threshold)
    logn = math.log(n)
    z = mu + eps * torch.exp(0.5 * lv)
    a = torch.exp(-lv)
    step = n if chunk is None else max(1, int(chunk))
    lqj, lqm = [], []
    for i0 in range(0, n, step):
        zi = z[i0: i0 + step, None, :]
        t = -0.5 * ((zi - mu[None]) ** 2 * a[None] + lv[None] + LOG_2PI)     # [c, n, Z]
        lqj.append(torch.logsumexp(t.sum(-1), 1) - logn)
        lqm.append((torch.logsumexp(t, 1) - logn).sum(-1))
    lq_joint, lq_marg = torch.cat(lqj), torch.cat(lqm)
    lq_cond = (-0.5 * ((z - mu) ** 2 * a + lv + LOG_2PI)).sum(-1)
    lp = (-0.5 * (z * z + LOG_2PI)).sum(-1)
    kl_per_dim = (0.5 * (mu * mu + torch.exp(lv) - lv - 1.0)).mean(0)
    mu_var = mu.var(0, unbiased=False)
    post_var = torch.exp(lv).mean(0)
    out = dict(rows=int(n), kl=float(kl_per_dim.sum()), kl_per_dim=kl_per_dim, mu_var=mu_var, post_var=post_var,
               active_units=int((mu_var > au_threshold).sum()), au_threshold=float(au_threshold),
               mi=float((lq_cond - lq_joint).mean()), tc=float((lq_joint - lq_marg).mean()),
               dwkl=float((lq_marg - lp).mean()), sampled_kl=float((lq_cond - lp).mean()))
    if return_rows:
        out.update(lq_joint=lq_joint, lq_marg=lq_marg, lq_cond=lq_cond, lp=lp)
    return out
