"""Shared inputs and bounds of the latent report tests (tests/unit/test_latent.py,
tests/gpu/test_latent_gpu.py): synthetic encoder rows ``mulv[n, 2Z]`` of three
kinds, the float64 oracle, and the per-quantity bound.

The bound is measured, not guessed: for an input, the error of the float32
torch oracle against the float64 oracle (same float32 inputs, same eps), per
quantity; a float32 implementation is held to ``MARGIN`` = 16 times that. The
margin covers the device's expf / logf at a few ulp, a different summation
order and the merge of the j-splits. It never comes from the code under test
(``bounds`` says where one run of the float32 oracle understates its own error
and what the measured error is floored by).
"""
import math

import numpy as np
import torch

from multidisttorch_amd.models import latent

MARGIN = 16.0
SCALARS = ("kl", "mi", "tc", "dwkl", "sampled_kl")
VECTORS = ("kl_per_dim", "mu_var", "post_var")
ROWS = ("lq_joint", "lq_marg", "lq_cond", "lp")


def _draw(n, Z, informative, seed):
    """``informative`` dimensions with mu ~ 1.5 N(0,1), lv ~ -3 +- 0.5; the rest
    collapsed: mu ~ 0.05 N(0,1), lv ~ -0.05 +- 0.02. Informative ones first."""
    g = np.random.RandomState(seed)
    mu = 0.05 * g.randn(n, Z)
    lv = -0.05 + 0.02 * g.randn(n, Z)
    mu[:, :informative] = 1.5 * g.randn(n, informative)
    lv[:, :informative] = -3.0 + 0.5 * g.randn(n, informative)
    return torch.from_numpy(np.concatenate([mu, lv], 1).astype(np.float32))


def overlap(n=40, Z=4, seed=5):
    """(a): one informative dimension whose posteriors overlap: mi well below log n."""
    return _draw(n, Z, 1, seed)


def mixed(n, Z, seed=7):
    """(b): Z/4 informative dimensions, 3Z/4 collapsed."""
    return _draw(n, Z, Z // 4, seed)


def sharp(n, Z, seed=9):
    """(c): lv falls linearly from 0 to -12 over the dimensions, the spread of mu
    grows from 0 to 3: joint log-densities from about -3e7 up to beyond +88.7,
    where a log-sum-exp without max subtraction overflows float32."""
    g = np.random.RandomState(seed)
    ramp = np.linspace(0.0, 1.0, Z)
    mu = g.randn(n, Z) * (3.0 * ramp)
    lv = np.broadcast_to(-12.0 * ramp, (n, Z))
    return torch.from_numpy(np.concatenate([mu, lv], 1).astype(np.float32))


def oracle(mulv, eps, dtype=torch.float64, au_threshold=0.01, chunk=None):
    """models/latent.py on float32 rows and eps, computed in ``dtype``."""
    Z = mulv.shape[1] // 2
    m = mulv.detach().cpu().to(dtype)
    return latent.latent_report(m[:, :Z], m[:, Z:], eps.detach().cpu().to(dtype), au_threshold, chunk=chunk,
                                return_rows=True)


def max_joint(mulv, eps):
    """The largest joint log-density sum_d t[i,j,d] of the input (float64)."""
    Z = mulv.shape[1] // 2
    m = mulv.double()
    mu, lv = m[:, :Z], m[:, Z:]
    z = mu + eps.double() * torch.exp(0.5 * lv)
    t = -0.5 * ((z[:, None] - mu[None]) ** 2 * torch.exp(-lv)[None] + lv[None] + math.log(2 * math.pi))
    return float(t.sum(-1).max())


def _err(a, b):
    if torch.is_tensor(a):
        return float((a.double() - b.double()).abs().max())
    return abs(float(a) - float(b))


U32 = 2.0 ** -24  # unit roundoff of float32


def bounds(mulv, eps):
    """(oracle64, {quantity: bound}) with bound = MARGIN * max(|oracle32 -
    oracle64|, U32 * scale) (max over the elements of a vector quantity).

    The floor: one run of the float32 oracle is one draw of its roundings, and
    in a mean over rows they can cancel far below the precision of the format
    (dwkl at n = 257, Z = 20: 2e-9 on a mean of float32 rows of magnitude 60).
    Such a figure measures luck, not the oracle's accuracy, so the measured
    error is never taken below one rounding of the largest float32 value that
    enters the quantity: the per-row values for the four row means, the
    quantity itself otherwise."""
    o64, o32 = oracle(mulv, eps), oracle(mulv, eps, torch.float32)
    row_scale = max(float(o64[k].abs().max()) for k in ROWS)
    out = {}
    for k in SCALARS + VECTORS + ROWS:
        v = o64[k]
        scale = float(v.abs().max()) if torch.is_tensor(v) else (abs(v) if k == "kl" else row_scale)
        out[k] = MARGIN * max(_err(o32[k], o64[k]), U32 * scale)
    return o64, out


def check(got, o64, bound, label="", rows=True):
    """Every scalar, per-dimension vector and (``rows``) per-row quantity of
    ``got`` against the float64 oracle within ``bound``; prints the achieved
    error next to the bound, returns {quantity: (error, bound)}."""
    rep = {}
    for k in SCALARS + VECTORS + (ROWS if rows else ()):
        g = got[k].detach().cpu() if torch.is_tensor(got[k]) else got[k]
        rep[k] = (_err(g, o64[k]), bound[k])
    print(f"latent {label}: " + "  ".join(f"{k} {e:.3g}/{b:.3g}" for k, (e, b) in rep.items()))
    bad = {k: v for k, v in rep.items() if not v[0] <= v[1]}
    assert not bad, f"{label}: error above 16x the float32 oracle's: {bad}"
    assert got["rows"] == o64["rows"] and got["active_units"] == o64["active_units"], label
    return rep
