"""Total-correlation penalty of a training batch (beta-TCVAE, Chen et al.).

``--latent-report`` measures the split of the KL term into mutual information,
total correlation and dimension-wise KL (models/latent.py); ``--beta`` scales
all three together. ``tc_weight`` weights the total correlation on its own,
estimated inside each minibatch of M rows from the stored ``mu, lv [M, Z]`` and
the step's own ``eps`` (the float32 ``z = mu + eps * exp(lv / 2)``)::

    t[i,j,d] = -0.5 * ((z[i,d] - mu[j,d])^2 * exp(-lv[j,d]) + lv[j,d] + log(2 pi))
    J[i]     = logsumexp_j sum_d t[i,j,d]          m[i,d] = logsumexp_j t[i,j,d]
    tc_batch = sum_i (J[i] - sum_d m[i,d]) + M * (Z - 1) * log M
    objective = BCE + kl_t * KL(with free bits) + tc_t * tc_batch

``tc_batch`` is ``M * latent_report(mu, lv, eps)["tc"]`` on the batch rows with
``n = M``, so models/latent.py defines the value and autograd through it the
gradient. ``tc_t = tc_weight * f_kl(t)`` follows the KL anneal's ramp and is 0
in evaluation, the importance-weighted pass and the latent report, which keep
the true ELBO terms. ``--beta 1 --tc-weight b-1`` is beta-TCVAE with
``alpha = gamma = 1``. The loss ring and ``epoch_loss`` keep meaning
``BCE + kl_t * KL``; the running sum of ``tc_batch`` is ``epoch_tc``.

The gradient in closed form, with ``q = z[i,d] - mu[j,d]``, ``a = exp(-lv[j,d])``
and ``w[i,j,d] = softmax_j(sum_d t)[i,j] - softmax_j(t[:,:,d])[i,j]``::

    g_z[i,d]  = sum_j w * (-q * a)    g_mu[j,d] = sum_i w * (q * a)    g_lv[j,d] = sum_i w * 0.5 * (q*q*a - 1)
    dmu_add[i,d] = g_z[i,d] + g_mu[i,d]       dlv_add[i,d] = g_z[i,d] * eps[i,d] * sd[i,d] / 2 + g_lv[i,d]

which is what csrc/kernels/vae_tc.hip computes (times ``tc_t``).
"""

from __future__ import annotations

import functools
import math
import warnings

import torch

from ..hpo import objective
from . import latent

__all__ = ["check_tc_weight", "tc_batch", "tc_closed_form"]


check_tc_weight = functools.partial(objective.check, "tc_weight")  # the penalty's weight: finite and >= 0


def tc_batch(mu: torch.Tensor, lv: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
    """``tc_batch`` of the rows as a 0-d tensor in their dtype (differentiable
    in ``mu`` and ``lv``): the sum over the rows of models/latent.py's
    ``lq_joint - lq_marg`` with ``n = M``."""
    with warnings.catch_warnings():  # the report also returns floats of its means: no gradient wanted there
        warnings.simplefilter("ignore", UserWarning)
        r = latent.latent_report(mu, lv, eps, return_rows=True)
    return (r["lq_joint"] - r["lq_marg"]).sum()


@torch.no_grad()
def tc_closed_form(mu: torch.Tensor, lv: torch.Tensor, eps: torch.Tensor):
    """(tc_batch, dmu_add, dlv_add): the value and its gradient with respect to
    ``mu`` and ``lv`` (through ``z`` too), unweighted, in the inputs' dtype."""
    M, Z = mu.shape
    sd = torch.exp(0.5 * lv)
    z = mu + eps * sd
    a = torch.exp(-lv)
    q = z[:, None, :] - mu[None]                                   # [i, j, d]
    t = -0.5 * (q * q * a[None] + lv[None] + latent.LOG_2PI)
    T = t.sum(-1)                                                  # [i, j]
    J = torch.logsumexp(T, 1)
    m = torch.logsumexp(t, 1)                                      # [i, d]
    value = (J - m.sum(-1)).sum() + M * (Z - 1) * math.log(M)
    w = torch.exp(T - J[:, None])[:, :, None] - torch.exp(t - m[:, None, :])
    qa = q * a[None]
    g_z = -(w * qa).sum(1)
    g_mu = (w * qa).sum(0)
    g_lv = (w * 0.5 * (q * qa - 1.0)).sum(0)
    return value, g_z + g_mu, g_z * eps * sd * 0.5 + g_lv
