"""Inputs, references and the tolerance rule of the mixture-prior tests (models/gmm.py; tests/unit/test_gmm.py,
tests/gpu/test_gmm_kernels.py, test_gmm_gpu.py).

Rows come from a planted K-component mixture whose means are about two standard deviations apart, so that
responsibilities are neither 0 nor 1. The tolerance of an output tensor is 8 times the largest absolute
deviation of the float32 run of the oracle from its float64 run on the same case (kernel and float32 torch run
chains of the same length in different orders; the factor covers the order), with a floor of 4 ulp of the
tensor's largest magnitude. Nothing comes from the kernels."""
import math

import torch

from multidisttorch_amd.models import gmm

# (n, Z, K)
SHAPES = [
    (33, 1, 1),        # the corner
    (37, 5, 3),        # below one MFMA tile
    (130, 20, 10),     # the MLP's Z; a row tail
    (257, 33, 2),      # one past two 16-column blocks: triangular block skipping
    (300, 64, 32),     # both limits
    (5000, 32, 10),    # several strips: the fixed-order fold
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
FACTOR = 8.0
_cache = {}


def planted(n, Z, K):
    """-> (rows [n, Z] float32, the planted parameters in float64)."""
    g = torch.Generator().manual_seed(1000 * K + 10 * Z + n)
    mu = torch.randn(K, Z, generator=g, dtype=torch.float64) * (1.5 / math.sqrt(Z))
    A = torch.randn(K, Z, Z, generator=g, dtype=torch.float64) / math.sqrt(Z)
    cov = A @ A.transpose(1, 2) + 0.5 * torch.eye(Z, dtype=torch.float64)
    comp = torch.arange(n)[torch.randperm(n, generator=g)] % K
    eps = torch.randn(n, Z, generator=g, dtype=torch.float64)
    z = mu[comp] + torch.einsum("nij,nj->ni", torch.linalg.cholesky(cov)[comp], eps)
    pi = torch.bincount(comp, minlength=K).double() / n
    return z.float(), dict(pi=pi, mu=mu, cov=cov)


def em_step(z, pi, mu, cov, reg=gmm.REG_COVAR):
    """One iteration of the oracle in the arguments' dtype: every tensor ``C.gmm_em_step`` returns."""
    W, c = gmm.gmm_prepare(pi, mu, cov, reg)
    r, ll = gmm.gmm_estep(z, mu, W, c)
    pi2, mu2, cov2 = gmm.gmm_mstep(z, r, mu, cov)
    return dict(W=W, c=c, r=r, ll=ll, pi=pi2, mu=mu2, cov=cov2)


def step_case(shape):
    """-> (z, float32 parameters after two float64 oracle iterations, float64 outputs, float32 outputs), once."""
    if shape not in _cache:
        n, Z, K = shape
        z = planted(n, Z, K)[0]
        p = gmm.gmm_init(z.double(), K)
        for _ in range(2):
            p = tuple(em_step(z.double(), *p)[k] for k in ("pi", "mu", "cov"))
        p32 = tuple(t.float() for t in p)
        _cache[shape] = (z, p32, em_step(z.double(), *(t.double() for t in p32)), em_step(z, *p32))
    return _cache[shape]


def tolerance(ref64, ref32):
    mag = float(ref64.abs().max())
    ulp = 2.0 ** (math.floor(math.log2(mag)) - 23) if mag > 0 else 0.0
    return max(FACTOR * float((ref32.double() - ref64).abs().max()), 4.0 * ulp)
