"""Ex-post Gaussian-mixture prior: a K-component full-covariance mixture fitted
by EM to draws from the aggregate posterior. The oracle.

The sample report scores what the decoder makes of the prior N(0, I). A poor
score has two possible causes, a poor decoder or a prior that does not match the
aggregate posterior q(z) = mean_x q(z|x). Ex-post density estimation (Ghosh et
al. 2020, "From Variational to Deterministic Autoencoders") removes the second:
fit a small mixture to latent codes of the training rows, sample it instead of
the prior, and score those samples with the same kernels. ``gap``, the test
codes' mean log-density under the mixture minus that under N(0, I), is what the
mismatch costs in nats.

One EM iteration on rows ``z [n, Z]`` with parameters ``pi [K]``, ``mu [K, Z]``,
``cov [K, Z, Z]``::

    prepare   L_k = chol(cov_k + reg I),  W_k = L_k^-1,
              c_k = log pi_k - sum_i log L_k[i, i] - Z/2 log 2 pi
    E         y = W_k (z_n - mu_k),  lp_nk = c_k - |y|^2 / 2,
              ll_n = logsumexp_k lp_nk,  r_nk = exp(lp_nk - ll_n)
    M         N_k = sum_n r_nk,  pi_k = N_k / n,  d = z_n - mu_old_k,
              mu_k = mu_old_k + sum r d / N_k,
              cov_k = sum r d d^T / N_k - (mu_k - mu_old_k)(mu_k - mu_old_k)^T

centred on the old mean, so that no large second moment is cancelled. A
component with ``N_k <= DEAD_WEIGHT n`` keeps its mean and covariance. The start
is deterministic (``gmm_init``) and the iteration count is fixed: a fit is a
function of (z, K, iters) only.

Everything here is plain torch, dtype-generic (float64 for the tests' oracle);
the trainers' ``torch`` backends run it in float32, and the HIP kernels
(csrc/kernels/gmm.hip) compute what these functions define.
"""

from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from ..ops.philox import reparam_eps

__all__ = ["GMM_STREAM", "MAX_K", "MAX_Z", "MAX_ROWS", "MAX_ITERS", "REG_COVAR", "DEAD_WEIGHT", "check_gmm_args",
           "gmm_init", "gmm_prepare", "gmm_estep", "gmm_mstep", "gmm_fit", "gmm_score", "gmm_counts", "gmm_sample",
           "gmm_fit_rows", "prior_score"]

GMM_STREAM = 7 << 28
MAX_K = 32
MAX_Z = 64
MAX_ROWS = 1 << 20
MAX_ITERS = 1000
REG_COVAR = 1e-4
DEAD_WEIGHT = 1e-6


def check_gmm_args(n: int, Z: int, K: int, iters: int):
    if int(K) != K or not 1 <= K <= MAX_K:
        raise ValueError(f"the mixture prior supports 1 <= components <= {MAX_K}, got K = {K!r}")
    if int(n) != n or not K < n <= MAX_ROWS:
        raise ValueError(f"the mixture prior supports K < rows <= {MAX_ROWS}, got {n!r} rows for K = {K}")
    if int(Z) != Z or not 1 <= Z <= MAX_Z:
        raise ValueError(f"the mixture prior supports 1 <= Z <= {MAX_Z} (a component's covariance is factored in one "
                         f"workgroup's LDS), got Z = {Z!r}")
    if int(iters) != iters or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"the mixture prior supports 0 <= EM iterations <= {MAX_ITERS}, got {iters!r}")


def gmm_mstep(z: torch.Tensor, r: torch.Tensor, mu_old: torch.Tensor, cov_old: torch.Tensor):
    """``(pi [K], mu [K, Z], cov [K, Z, Z])`` from responsibilities ``r [n, K]``, centred on ``mu_old``."""
    n, K = r.shape
    N = r.sum(0)
    mu, cov = mu_old.clone(), cov_old.clone()
    for k in range(K):
        if not float(N[k]) > DEAD_WEIGHT * n:
            continue
        d = z - mu_old[k]
        rd = r[:, k, None] * d
        dm = rd.sum(0) / N[k]
        mu[k] = mu_old[k] + dm
        cov[k] = rd.t() @ d / N[k] - dm[:, None] * dm[None, :]
    return N / n, mu, cov


def gmm_init(z: torch.Tensor, K: int):
    """The deterministic start: equal weights, means at K evenly spaced rows, every covariance the population
    covariance of all rows."""
    n, Z = z.shape
    zero = z.new_zeros(1, Z)
    _, _, cov = gmm_mstep(z, z.new_ones(n, 1), zero, z.new_zeros(1, Z, Z))
    mu = z[[((2 * k + 1) * n) // (2 * K) for k in range(K)]].clone()
    return z.new_full((K,), 1.0 / K), mu, cov.expand(K, Z, Z).clone()


def gmm_prepare(pi: torch.Tensor, mu: torch.Tensor, cov: torch.Tensor, reg: float = REG_COVAR):
    """``(W [K, Z, Z], c [K])``: the inverse Cholesky factors and the log-density constants."""
    K, Z = mu.shape
    eye = torch.eye(Z, dtype=cov.dtype, device=cov.device)
    L, info = torch.linalg.cholesky_ex(cov + reg * eye)
    if bool((info != 0).any()) or not bool(torch.isfinite(L).all()):
        raise ValueError(f"a mixture component's covariance is not positive definite (components "
                         f"{(info != 0).nonzero().flatten().tolist()})")
    W = torch.linalg.solve_triangular(L, eye.expand(K, Z, Z), upper=False)
    c = torch.log(pi) - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1) - 0.5 * Z * math.log(2.0 * math.pi)
    return W, c


def gmm_estep(z: torch.Tensor, mu: torch.Tensor, W: torch.Tensor, c: torch.Tensor):
    """``(r [n, K], ll [n])``: responsibilities and per-row log-density."""
    lp = torch.stack([c[k] - 0.5 * (((z - mu[k]) @ W[k].t()) ** 2).sum(1) for k in range(mu.shape[0])], 1)
    ll = torch.logsumexp(lp, 1)
    return torch.exp(lp - ll[:, None]), ll


def gmm_fit(z: torch.Tensor, K: int, iters: int) -> Dict[str, torch.Tensor]:
    """``dict(pi, mu, cov, ll_history [iters + 1])``; ``ll_history[t]`` is the mean log-density of the rows
    under the parameters before iteration ``t``, the last entry under the returned ones."""
    n, Z = z.shape
    check_gmm_args(n, Z, K, iters)
    pi, mu, cov = gmm_init(z, K)
    hist = []
    for _ in range(iters):
        W, c = gmm_prepare(pi, mu, cov)
        r, ll = gmm_estep(z, mu, W, c)
        hist.append(ll.mean())
        pi, mu, cov = gmm_mstep(z, r, mu, cov)
    hist.append(gmm_score(z, dict(pi=pi, mu=mu, cov=cov)).mean())
    return dict(pi=pi, mu=mu, cov=cov, ll_history=torch.stack(hist))


def gmm_score(z: torch.Tensor, params) -> torch.Tensor:
    """``ll [n]``: the rows' log-density under the mixture."""
    W, c = gmm_prepare(params["pi"], params["mu"], params["cov"])
    return gmm_estep(z, params["mu"], W, c)[1]


def prior_score(z: torch.Tensor) -> torch.Tensor:
    """``lp [n]``: the rows' log-density under N(0, I)."""
    return -0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * math.log(2.0 * math.pi)


def gmm_counts(pi, nb: int) -> np.ndarray:
    """Rows per component of a stratified draw: the largest-remainder rounding of ``pi_k nb``, ties to the lower k."""
    q = np.asarray(pi, dtype=np.float64)
    q = q / q.sum() * nb
    cnt = np.floor(q).astype(np.int64)
    order = np.argsort(-(q - cnt), kind="stable")
    cnt[order[: nb - int(cnt.sum())]] += 1
    return cnt


def gmm_sample(params, nb: int, seed: int) -> torch.Tensor:
    """``z [nb, Z]`` float32: a stratified draw, rows ordered by component, ``z_j = mu_k + L_k eps_j``."""
    pi, mu, cov = (params[k].detach().double().cpu() for k in ("pi", "mu", "cov"))
    Z = mu.shape[1]
    L = torch.linalg.cholesky(cov + REG_COVAR * torch.eye(Z, dtype=torch.float64))
    comp = torch.from_numpy(np.repeat(np.arange(pi.numel()), gmm_counts(pi.numpy(), nb)))
    eps = torch.from_numpy(reparam_eps(nb, Z, seed, GMM_STREAM, 0)).double()
    return (mu[comp] + torch.einsum("nij,nj->ni", L[comp], eps)).float()


def gmm_fit_rows(mu: torch.Tensor, lv: torch.Tensor, seed: int, step: int = 1) -> torch.Tensor:
    """The codes a mixture is fitted to (``step`` 1) or scored on (``step`` 2): one draw per row from its
    posterior, ``z_i = mu_i + exp(lv_i / 2) eps_i``. Not the means: collapsed dimensions then have variance
    near 1 and the covariances stay well conditioned."""
    n, Z = mu.shape
    eps = torch.from_numpy(reparam_eps(n, Z, seed, GMM_STREAM, step)).to(device=mu.device, dtype=mu.dtype)
    return mu + torch.exp(0.5 * lv) * eps
