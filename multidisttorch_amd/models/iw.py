"""Importance-weighted test log-likelihood (Burda et al., IWAE): the oracle.

A beta-independent score for comparing trials of a sweep whose axis is beta
itself. For row i with encoder outputs (mu, lv) and samples k = 0..K-1::

    sd = exp(lv / 2),  z = mu + eps * sd
    bce[k, i]       clamped logit-form BCE of decode(z[k, i]) against x[i], summed over the pixels
    logw[k, i]      = -bce[k, i] + sum_c(-z^2/2 + eps^2/2 + lv/2)     (log p(x, z) - log q(z | x))
    row_nll[i]      = -(logsumexp_k logw[k, i] - log K)
    row_neg_elbo[i] = -mean_k logw[k, i]

beta and the lr / KL schedules do not enter. The noise is Philox with the trial
seed as key, stream word ``IW_STREAM`` (no ``rng_stream``: every replica of a
group computes the same number), the 0-based batch index of the pass as step
words and counter ``(k*B + i)*Z + c`` with B the trainer's batch size, so a
tail batch draws what a full batch would and a pass is a pure function of
(weights, data, seed, K).

Everything here is plain torch ops, dtype-generic (float64 for the tests'
oracle); the trainers' ``torch`` backends run these same functions and the HIP
kernels (csrc/kernels/vae_iw.hip) implement them.
"""

from __future__ import annotations

import math
from typing import Callable, Dict, Tuple

import numpy as np
import torch

from ..ops.philox import reparam_eps
from .mlp_vae import _bce_terms, _w

__all__ = ["IW_STREAM", "check_iw_args", "default_chunk", "iw_eps", "iw_prior_term", "iw_log_weights", "iw_reduce",
           "mlp_encode", "mlp_decode_logits", "mlp_iw_log_weights"]

IW_STREAM = 1 << 29
# default chunk: at most this many virtual rows (samples x batch rows) per launch group
CHUNK_ROWS = 8192


def check_iw_args(k: int, B: int, Z: int):
    if int(k) != k or k < 1:
        raise ValueError(f"iw samples must be an integer >= 1, got {k!r}")
    if k * B * Z > 2 ** 32:
        raise ValueError(f"k*B*Z = {k * B * Z} exceeds the 2^32 Philox counter range of one batch")


def default_chunk(k: int, B: int, chunk_samples=None) -> int:
    """Samples per chunk: the caller's, else as many as keep S*B <= CHUNK_ROWS."""
    if chunk_samples is not None:
        if int(chunk_samples) < 1:
            raise ValueError("chunk_samples must be >= 1")
        return min(int(chunk_samples), k)
    return max(1, min(k, CHUNK_ROWS // B))


def iw_eps(k: int, B: int, Z: int, seed: int, batch: int) -> np.ndarray:
    """eps[K, B, Z] (float32) of batch ``batch`` of a pass, as the kernels draw it."""
    return reparam_eps(k * B, Z, seed, IW_STREAM, batch).reshape(k, B, Z)


def iw_prior_term(z: torch.Tensor, eps: torch.Tensor, lv: torch.Tensor) -> torch.Tensor:
    """log p(z) - log q(z | x) summed over the latent axis (the 2 pi terms cancel)."""
    return (-0.5 * z * z + 0.5 * eps * eps + 0.5 * lv).sum(-1)


def iw_log_weights(mu: torch.Tensor, lv: torch.Tensor, eps: torch.Tensor, x: torch.Tensor,
                   decode_logits: Callable[[torch.Tensor], torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """logw[K, M] and z[K, M, Z] from mu, lv [M, Z], eps [K, M, Z], x [M, D] and
    ``decode_logits``: [K*M, Z] -> [K*M, D] logits in x's pixel order."""
    K, M, Z = eps.shape
    z = mu + eps * torch.exp(0.5 * lv)
    t = decode_logits(z.reshape(K * M, Z)).reshape(K, M, -1)
    bce = _bce_terms(t, x.unsqueeze(0)).sum(-1)
    return -bce + iw_prior_term(z, eps, lv), z


def iw_reduce(logw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row_nll[M], row_neg_elbo[M]) from logw[K, M]."""
    K = logw.shape[0]
    return -(torch.logsumexp(logw, 0) - math.log(K)), -logw.mean(0)


# ---------------------------------------------------------------- MLP-VAE
def mlp_encode(v: Dict[str, torch.Tensor], x: torch.Tensor):
    W1, b1, W2, b2 = _w(v)[:4]
    Z = W2.shape[0] // 2
    mulv = torch.relu(x @ W1.t() + b1) @ W2.t() + b2
    return mulv[:, :Z], mulv[:, Z:]


def mlp_decode_logits(v: Dict[str, torch.Tensor], z: torch.Tensor) -> torch.Tensor:
    W3, b3, W4, b4 = _w(v)[4:]
    return torch.relu(z @ W3.t() + b3) @ W4.t() + b4


def mlp_iw_log_weights(v: Dict[str, torch.Tensor], x: torch.Tensor, eps: torch.Tensor):
    """(logw[K, M], z[K, M, Z]) of the MLP-VAE with parameter views ``v``."""
    mu, lv = mlp_encode(v, x)
    return iw_log_weights(mu, lv, eps, x, lambda z: mlp_decode_logits(v, z))
