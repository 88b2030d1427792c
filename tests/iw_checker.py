"""Shared checker of the importance-weighted pass's kernels (iw_sample_k,
iw_dec_bce_k, iw_reduce_k of csrc/kernels/vae_iw.hip; iw_reparam_k, iw_row_bce_k
of conv_iw.hip): float64 oracles, per-element bounds and the named inputs of
tests/unit/test_iw_checker.py (CPU: the checker is not vacuous) and
tests/gpu/test_iw_kernels.py (the kernels through their bindings).

Let u = 2^-24 (``mlp_checker.U``). The library functions are taken at their
documented HIP accuracy (expf, logf, log1pf 1 ulp = 2 u; division 2.5 ulp = 5 u),
a sum of n f32 numbers in any fixed order with at most d additions on the path
of a term carries ``d u sum|terms|`` (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2), and an input's bound is carried through the
formula's partial derivatives. NO bound of this module is measured.

* eps: ``ops.philox.reparam_eps(K B, Z, seed, IW_STREAM, step - 1)``, row
  ``(k0 + s) B + i`` with B the trainer's batch size (not the batch's row count
  M), at the project's rtol = atol = 1e-5, keyed with ``step - 1`` of the
  state the kernel is handed (the 0-based batch index).
* z = mu + eps sd, sd = expf(lv / 2) (lv / 2 is exact): ``eps sd`` carries
  2 u (expf) + u, the sum u: b_z = 4 u (|mu| + |eps sd|). z16 is compared
  BITWISE with ``z32.to(bfloat16)``.
* prior[v] = sum_c p_c, p_c = -z^2/2 + eps^2/2 + lv/2 from the f32 mulv and eps
  the device holds. With T_c = z^2/2 + eps^2/2 + |lv|/2:
    - the z the kernel squares lies within b_z of the oracle's:
      |z| b_z + b_z^2 / 2;
    - z z and eps eps round once each (the factors 0.5 are exact), the two
      additions once each of a partial sum of magnitude <= T_c: 3 u T_c to first
      order, taken as 4 u T_c (second order, and the rounded z in the square);
    - the Z terms are added serially in latent order by one thread: at most Z
      additions on a term's path, Z u sum_c T_c.
  b_prior = sum_c (|z| b_z + b_z^2 / 2 + 4 u T_c) + Z u sum_c T_c.
* row BCE: the per-pixel bound b_loss of ``conv_small_checker.bce_ref`` (8 u of
  the formula's terms, plus TINY where a term underflows) summed over the row,
  plus the sum bound of the kernel's order over the non-negative terms:
    - conv (iw_row_bce_k): a strided per-thread chain of ceil(P / 256) terms,
      then the fixed 256-lane tree (6 + 2 levels): (ceil(P / 256) + 8) u sum;
    - MLP (iw_dec_bce_k): a lane's chain over its ceil(ceil(D / 16) / 8) column
      tiles, a 4-level butterfly over the 16 lanes of a row, the 8 waves
      serially: (ceil(D / 128) + 12) u sum. The logits are
      ``gemm_ref(h3_device, W4^T, b4)`` with their bound b_t; the term is
      1-Lipschitz in t (|d term / d t| = |p - x| <= 1, min() included), so
      sum_j b_t[j] is added.
* reduce (iw_reduce_k). Inputs prior, bce (f32); lw_k = fl(prior - bce) is one
  rounding, u |lw_k|, part of the input bound b_lw below. Comparisons are
  exact, so the running maximum m is the exact maximum of the lw_k. A sample
  at distance d under the running maximum enters as expf(fl(lw - m)): u d from
  the subtraction (relative, through exp) + 2 u. A new maximum rescales the sum
  by expf(fl(m - lw)), (2 + d_j) u again, then one multiplication and one
  addition (u each; an else-branch step has the addition only). Sample k, at
  distance Delta_k under the FINAL maximum, has gone through r_k rescales whose
  distances add up, with its own, to Delta_k, and through at most K - 1 steps
  of two roundings: its share p_k = e^-Delta_k / ss of the scaled sum carries
  (2 + 2 r_k + 2 (K - 1) + Delta_k) u <= (4 K + Delta_k) u relative. Summed
  with the weights p_k (sum 1): 4 K u + u sum_k Delta_k e^-Delta_k / ss, and
  since ss >= 1, Delta <= D = max - min and x e^-x <= 1/e:
      rho = (4 K + min(D, K / e) + 4) u            (the + 4: second order)
  is the scaled sum's relative error, so logf(ss) errs by rho + 2 u |log ss|.
  ``m + log ss`` and ``- log K`` round once each, of values near |m|, and
  logf((float)K) carries 2 u log K + u log K:
      b_nll = rho + 2 u |log ss| + u |m + log ss| + u |nll| + 3 u log K + max_k b_lw.
  At |m| ~ 540 the two additions dominate: 2 u |m| ~ 6.4e-5 absolute (the
  end-to-end tests allow 1e-2). logsumexp is 1-Lipschitz in the sup norm, hence
  max_k b_lw, with no first-order argument.
  row_neg_elbo = -(serial sum of the K lw) / K: (K - 1) u sum|lw| / K for the
  sum and 5 u for the division, together <= (K + 4) u sum|lw| / K, plus the
  mean of b_lw.
* totals: the state's nll / neg_elbo are double sums (per-thread sums in row
  order, a fixed tree, one addition per batch) of the f32 rows the device
  wrote: against ``rows.double().sum()`` at n 2^-52 sum|row| for n rows.

All results are error/bound ratios (``mlp_checker.ratio``): pass means <= 1.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from tests.conv_small_checker import EPS_TOL, TINY, bce_ref, gen
from tests.mlp_checker import U, check_gemm, gemm_ref, ratio

IW_STREAM = 1 << 29
LANES = 256          # threads of iw_row_bce_k and of iw_reduce_k
CHUNK_ROWS = 8192    # models/iw.py: the default chunk keeps S * B within this


# ------------------------------------------------------------------- cases ----
# iw_reparam (M, B, Z, k0, S): Z = 256 is the kernel's limit (four trips of its 64-lane loop)
REPARAM_CASES = [(5, 32, 8, 0, 6), (37, 48, 24, 3, 1), (3, 16, 256, 1, 5), (4, 16, 1, 0, 4), (16, 16, 32, 49, 1)]
REPARAM_STEPS = (1, 3)   # state steps: batch index 0 and 2
# iw_row_bce (V, M, P)
ROW_BCE_CASES = [(30, 5, 784), (1, 1, 1), (37, 37, 100), (4, 2, 16384), (70, 7, 300)]
# iw_reduce (M, B, K, S): a full batch of B rows, then a tail of M
REDUCE_CASES = [(1, 1, 1, 1), (21, 32, 5, 2), (5, 32, 50, 6), (300, 300, 7, 3), (257, 512, 4, 4)]
PATTERNS = ("spread10", "ascending", "descending", "max_last", "equal", "spread200", "bce1e6")
# the MLP pass (B, tail, D, H, Z, K, chunk_samples, scaled weights)
MLP_RUNS = {
    "b128_k50": (128, 37, 784, 400, 20, 50, None, True),   # one chunk, V = 6400 and 1850
    "b128_k7c3": (128, 37, 784, 400, 20, 7, 3, True),
    "ragged": (48, 37, 100, 36, 12, 5, None, True),
    "h496": (32, 17, 256, 496, 32, 5, 2, True),            # H at the pass's limit
    "tiny": (16, 5, 20, 20, 4, 3, 1, True),
    "b300": (300, 263, 32, 32, 4, 5, None, True),          # rows >= 256 in the reduce
    "b4096": (4096, 4081, 32, 32, 4, 3, None, False),      # S = 2
}
MLP_SCALE = 6.0      # fc21 / fc22, as tests/gpu/test_tc_penalty_gpu.py
LOGIT_PEAK = 150.0   # fc4 is scaled so that the largest |logit - bias| of batch 0 is this


def chunks(K: int, S: int):
    """[(k0, s)]: the samples of a batch in chunks of S, the last one short."""
    return [(k0, min(S, K - k0)) for k0 in range(0, K, S)]


def default_chunk(K: int, B: int, chunk=None) -> int:
    return min(chunk, K) if chunk is not None else max(1, min(K, CHUNK_ROWS // B))


# ------------------------------------------------------------------ inputs ----
def reparam_mulv(M: int, Z: int, seed: int = 0) -> torch.Tensor:
    """mulv [M, 2Z] f32: mu ~ U(-3, 3), lv ~ U(-8, 4)."""
    g = gen(seed)
    mu = torch.rand(M, Z, generator=g) * 6 - 3
    lv = torch.rand(M, Z, generator=g) * 12 - 8
    return torch.cat([mu, lv], 1).contiguous()


PLANTED = (0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 200.0, -200.0)


def row_bce_inputs(V: int, M: int, P: int, seed: int = 0):
    """(logits [V, P], images [M, P]) f32. Logits: N(0, 3) with PLANTED under
    targets 0, 1 and a grey at 27 positions of every row (as many as P holds).
    Even image rows are exact {0, 1}, odd ones greys with a 0 and a 1."""
    g = gen(seed)
    t = 3.0 * torch.randn(V, P, generator=g)
    x = torch.rand(M, P, generator=g)
    x[0::2] = (x[0::2] > 0.5).float()
    if P >= 2:
        x[1::2, 0], x[1::2, P - 1] = 0.0, 1.0
    n = min(P, 3 * len(PLANTED))
    for v in range(V):
        pos = (7 * v + torch.arange(n)) % P
        t[v, pos] = torch.tensor([PLANTED[k // 3] for k in range(n)])
    for i in range(M):   # the targets under row i's own planted logits (virtual row v = i)
        pos = (7 * i + torch.arange(n)) % P
        x[i, pos] = torch.tensor([((0.0, 1.0, 0.25) if i % 2 else (0.0, 1.0, 1.0))[k % 3] for k in range(n)])
    return t.contiguous(), x.contiguous()


def reduce_inputs(pattern: str, K: int, M: int, seed: int = 0):
    """(prior [K, M], bce [K, M]) f32 whose difference lw follows ``pattern``."""
    g = gen(seed)
    prior = -15.0 + 3.0 * torch.randn(K, M, generator=g)
    base = -540.0 - 10.0 * torch.rand(K, M, generator=g)
    if pattern == "spread10":
        tgt = base
    elif pattern == "ascending":      # a new maximum at every sample
        tgt = base.sort(0).values
    elif pattern == "descending":
        tgt = base.sort(0, descending=True).values
    elif pattern == "max_last":       # the maximum in the last sample of the last chunk
        tgt = base.clone()
        tgt[K - 1] = -539.0 + torch.rand(M, generator=g)
    elif pattern == "equal":          # bitwise equal lw over k
        tgt = base[:1].expand(K, M)
        prior = prior[:1].expand(K, M)
    elif pattern == "spread200":      # one sample at -540, the others 100 .. 200 nats below
        tgt = -740.0 + 100.0 * torch.rand(K, M, generator=g)
        tgt[torch.arange(M) % K, torch.arange(M)] = -540.0
    elif pattern == "bce1e6":         # BCE sums at 128 x 128 clamp scale
        tgt = base - 1.6e6
    else:
        raise ValueError(pattern)
    bce = (prior.double() - tgt.double()).float()
    return prior.contiguous(), bce.contiguous()


# ----------------------------------------------------------------- oracles ----
def eps_ratio(got, B: int, Z: int, k0: int, seed: int, state_step: int) -> float:
    """got [S, M, Z]: samples k0 .. k0 + S - 1 of rows 0 .. M - 1 of a batch of B."""
    from multidisttorch_amd.ops.philox import reparam_eps

    S, M, _ = got.shape
    want = torch.from_numpy(reparam_eps((k0 + S) * B, Z, seed, IW_STREAM, state_step - 1).astype(np.float64))
    want = want.view(k0 + S, B, Z)[k0:, :M]
    err = (got.double() - want).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    return float((err / (EPS_TOL + EPS_TOL * want.abs())).max())


def reparam_ref(mulv, eps):
    """float64 (z [S, M, Z], b_z, prior [S, M], b_prior) from mulv [M, 2Z] and eps [S, M, Z]."""
    Z = mulv.shape[-1] // 2
    mu, lv, e = mulv[:, :Z].double(), mulv[:, Z:].double(), eps.double()
    es = e * torch.exp(0.5 * lv)
    z = mu + es
    b_z = 4 * U * (mu.abs() + es.abs())
    T = 0.5 * z * z + 0.5 * e * e + 0.5 * lv.abs()
    prior = (-0.5 * z * z + 0.5 * e * e + 0.5 * lv).sum(-1)
    b_prior = (z.abs() * b_z + 0.5 * b_z * b_z + 4 * U * T).sum(-1) + Z * U * T.sum(-1)
    return z, b_z, prior, b_prior


def conv_depth(P: int) -> int:
    return -(-P // LANES) + 8


def mlp_depth(D: int) -> int:
    return -(-D // 128) + 12


def row_bce_ref(t, x, depth: int, b_t=None, want_clamped: bool = False):
    """float64 (bce [V], bound [V]) of logits t [V, P] against image row v % M of
    x [M, P]; ``want_clamped``: also the number of pixels at which the 100 clamp bites."""
    V, M = t.shape[0], x.shape[0]
    xv = x[torch.arange(V) % M]
    r = bce_ref(t, xv)
    ref = r["loss"].sum(-1)
    bound = r["b_loss"].sum(-1) + depth * U * ref
    if b_t is not None:
        bound = bound + b_t.sum(-1)
    if want_clamped:
        td, xd = t.double(), xv.double()
        return ref, bound, int((((td > 100) & (xd < 1)) | ((td < -100) & (xd > 0))).sum())
    return ref, bound


def lw_ref(prior, bce, b_prior=None, b_bce=None):
    """float64 lw = prior - bce and its bound: the f32 subtraction's rounding plus the inputs' bounds."""
    lw = prior.double() - bce.double()
    b = U * lw.abs()
    if b_prior is not None:
        b = b + b_prior
    if b_bce is not None:
        b = b + b_bce
    return lw, b


def reduce_ref(lw, b_lw=None, K=None):
    """float64 (row_nll [M], row_neg_elbo [M], b_nll, b_ne) of lw [k, M];
    ``K``: the divisor when it is not the number of rows of ``lw``."""
    n = lw.shape[0]
    K = n if K is None else K
    lw = lw.double()
    m = lw.max(0).values
    D = m - lw.min(0).values
    ss = torch.exp(lw - m).sum(0)
    lse = m + torch.log(ss)
    nll = -(lse - math.log(K))
    ne = -lw.sum(0) / K
    mag = lw.abs().sum(0) / K
    rho = (4 * n + torch.clamp(D, max=n / math.e) + 4) * U
    b_nll = rho + 2 * U * torch.log(ss).abs() + U * lse.abs() + U * nll.abs() + 3 * U * math.log(K)
    b_ne = (n + 4) * U * mag
    if b_lw is not None:
        b_nll = b_nll + b_lw.max(0).values
        b_ne = b_ne + b_lw.sum(0) / K
    return nll, ne, b_nll, b_ne


def totals_ratio(total: float, rows) -> float:
    """The state's double total against the double sum of the f32 rows the device wrote."""
    r = rows.double()
    if not bool(torch.isfinite(r).all()) or not math.isfinite(total):
        return math.inf
    bound = r.numel() * 2.0 ** -52 * float(r.abs().sum())
    err = abs(total - float(r.sum()))
    return err / bound if bound > 0 else (0.0 if err == 0 else math.inf)


__all__ = ["U", "TINY", "IW_STREAM", "ratio", "gemm_ref", "check_gemm", "gen", "REPARAM_CASES", "REPARAM_STEPS",
           "ROW_BCE_CASES", "REDUCE_CASES", "PATTERNS", "MLP_RUNS", "MLP_SCALE", "LOGIT_PEAK", "chunks",
           "default_chunk", "reparam_mulv", "row_bce_inputs", "reduce_inputs", "eps_ratio", "reparam_ref",
           "conv_depth", "mlp_depth", "row_bce_ref", "lw_ref", "reduce_ref", "totals_ratio"]
