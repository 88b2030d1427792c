"""Shared checker of the conv-VAE step's small kernels (csrc/kernels/conv_bf16.hip,
conv_small.h, colsum_body of conv_igemm_dev.h): float64 oracles, per-element
bounds and the inputs of tests/unit/test_conv_small_checker.py (CPU: the
checker is not vacuous) and tests/gpu/test_conv_small_kernels.py (the kernels).

Let u = 2^-24 (``mlp_checker.U``). Every bound below follows the rule
``mlp_checker`` already uses: an input's bound carried through the formula's
partial derivatives, plus ``8 u sum|terms|`` for the formula's own roundings.
The library functions are taken at their documented HIP accuracy (expf, log1pf,
sqrtf 1 ulp = 2 u; division 2.5 ulp = 5 u); with them the rule suffices for
every formula here, so NO bound of this module is measured:

* z = mu + eps sd, sd = expf(lv / 2): ``eps sd`` carries 2 u (expf) + u, the
  sum u: <= 4 u (|mu| + |eps sd|).
* KLD term k = 1 + lv - mu^2 - sd^2 (the kernels sum k and scale the block sum
  by -0.5, exactly): sd^2 carries 2 * 2 u + u, each of the other three
  operations u of its partial result: <= 6 u (1 + |lv| + mu^2 + sd^2).
* A block's partial (kld_part, part, gpart) is a sum of 256 lane values in a
  fixed tree: the lane bounds added, plus the any-order bound
  ``(256 + 4) u sum|lane value|`` (Higham, section 4.2).
* dm = g + beta mu: <= 2 u (|g| + |beta mu|). dl = 0.5 g eps sd +
  0.5 beta (sd^2 - 1): <= 5 u |0.5 g eps sd| + 8 u 0.5 |beta| (sd^2 + 1)
  (the same expression as ``mlp_checker.check_backward``); a bound on g (a
  split-K sum) enters through d dm / d g = 1 and d dl / d g = 0.5 eps sd.
* p = 1 / (1 + expf(-t)): the denominator carries 2 u e + u (1 + e), the
  division 5 u: <= 8 u p, plus 2^-126 where the result leaves the normal range
  (expf(88.8) overflows: p = 0 against 2.7e-39). g = p - x: <= 8 u (p + |x|).
* BCE, sp = max(t, 0) + log1pf(expf(-|t|)), loss = x min(sp - t, 100) +
  (1 - x) min(sp, 100): the log term l carries 2 u (expf, through
  e / ((1 + e) log1p(e)) <= 1) + 2 u, sp another u sp; ``sp - t`` CANCELS for
  t > 0 (the kernel's formula, not the oracle's), which leaves u (sp + |t|)
  absolute; min() is 1-Lipschitz. In all <= 8 u (x (sp + |t|) + (1 - x) sp),
  plus 2^-126 where a term underflows (softplus(-88.8) = 2.7e-39).
* Split-K slab sum over ks slices (+ bias): ``(ks + 4) u (sum|slab| + |bias|)``,
  the any-order bound, since the row form, the element form and a job form
  may each order the slices differently.
* Adam (adam_common.h ``adam_update``), every operation with its own u, sqrt 2 u,
  the two divisions 5 u, the f32 roundings of step_size, bc2s and lr one u each:
    gr = g gs (+ wd p coupled)      b_gr = 2 u (|g gs| + |wd p|)
    p1 = p (1 - lr wd) decoupled     b_p1 = 4 u |p|
    m' = m + omb1 (gr - m)           b_m  = u (|m'| + omb1 (|gr| + |m|)) + omb1 b_gr
    v' = b2 v + omb2 gr^2            b_v  = u (v' + omb2 gr^2 + b2 v) + 2 omb2 |gr| b_gr
    den = sqrt(v') / bc2s + eps      b_den = 8 u sqrt(v') / bc2s + b_v / (2 sqrt(v') bc2s) + u den
    p' = p1 - ss m' / den            b_p  = b_p1 + u |p'| + |ss m' / den| (7 u + b_den / den) + ss b_m / den
  (first order in b_v / v': the tests keep v' >= 1e-3.) The oracle takes the
  hyper-parameters as the kernel reads them from HParams (f32 beta1, beta2,
  eps, weight_decay, grad_scale), lr_t = lr * f_lr(t) and beta^t =
  pow(beta, t) in double as TrialState seeds them, and the two moment weights
  by the conv kernels' documented convention ``float32(1) - float32(beta)``
  (adam_common.h, AdamC::omb1/omb2): a modelled convention, not a tolerance.
* bf16 twins (z16, dmulv16, w16) are compared BITWISE with ``.to(bfloat16)`` of
  the f32 value the same launch wrote. dlog16 has no f32 twin: one bf16
  rounding (2^-8 relative) of the float64 value plus the f32 bound.
* Philox noise: ``ops.philox.reparam_eps`` at rtol = atol = 1e-5, keyed with
  ``step - 1`` of the state the kernel is handed.

All results are error/bound ratios (``mlp_checker.ratio``): pass means <= 1.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from tests.mlp_checker import U, ratio

TINY = 2.0 ** -126    # smallest normal f32 / bf16: absolute slack where a result underflows
BF16_U = 2.0 ** -8    # bf16 unit roundoff (8 significand bits, round to nearest)
LANES = 256           # threads (lane values) per block sum
EPS_TOL = 1e-5        # mlp_checker's rtol = atol of the Philox noise
BF16_FILL = 24576.0   # out-of-band poison of bf16 buffers (exactly representable, never produced)


# ------------------------------------------------------ domain (conv_small.h) ----
def splitk_rp(ks: int) -> int:
    rp = 1
    while rp < 64 and rp * 4 < ks:
        rp *= 2
    return rp


def rows_ok(Z: int) -> bool:
    """The row form of the split-K combines: one 256-thread block per sample
    row, thread c owning column c, so Z a power of two in [8, 256]."""
    return 8 <= Z <= 256 and Z & (Z - 1) == 0


ROW_Z = (8, 32, 64, 256, 512)   # powers of two, swept with row_ks(); 512 is served by the element form
                                # (the row form used to admit it and left columns 256.. unwritten)
ELEM_Z = (24, 40)
ELEM_KS = (1, 5, 17, 300)       # splitk_rp = 1, 2, 8, 64


def row_ks(Z: int, fwd: bool):
    """k-slice counts around the unrolled round of combine_rows_partial: RG =
    256 / LW row groups of LW = (2Z | Z) / 4 float4 lanes; 16 RG slices per
    unrolled round: tail loop only, one round exactly, one round + tail, two + tail."""
    lw = (2 * Z if fwd else Z) // 4
    rg = max(1, 256 // lw)
    return sorted({1, 3, rg, 16 * rg, 16 * rg + 1, 33 * rg + 5})


def block_owners(B: int, Z: int, ks=None):
    """Element indices (into the flat [B * Z]) whose KLD terms each block sums:
    stand-alone reparam (ks None): 256 consecutive elements; row form: sample
    row b; element form: 256 / splitk_rp(ks) consecutive elements."""
    n = B * Z
    if ks is None:
        cnt = LANES
    elif rows_ok(Z):
        cnt = Z
    else:
        cnt = LANES // splitk_rp(ks)
    return [torch.arange(s, min(n, s + cnt)) for s in range(0, n, cnt)]


# ------------------------------------------------------------------ inputs ----
def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def reparam_inputs(B: int, Z: int, seed: int = 0) -> torch.Tensor:
    """mulv [B, 2Z] f32: mu ~ N(0, 1), lv ~ U(-6, 3)."""
    g = gen(seed)
    mu = torch.randn(B, Z, generator=g)
    lv = torch.rand(B, Z, generator=g) * 9 - 6
    return torch.cat([mu, lv], 1).contiguous()


def slab_inputs(ks: int, B: int, Z: int, fwd: bool, seed: int = 0):
    """(slab [ks + 1, B, W] f32 with a NaN slice beyond ks, bias [W]); W = 2Z
    forward (sums to mu ~ N(0, 1) | lv ~ N(0, 1.5^2)), Z backward (dz ~ N(0, 1))."""
    g = gen(seed)
    W = 2 * Z if fwd else Z
    s = torch.randn(ks, B, W, generator=g) / math.sqrt(ks)
    if fwd:
        s[:, :, Z:] *= 1.5
    slab = torch.cat([s, torch.full((1, B, W), float("nan"))], 0).contiguous()
    bias = 0.5 * torch.randn(W, generator=g)
    return slab, bias


PLANTED = (0.0, 20.0, 88.8, 95.0, 120.0)


def bce_inputs(B: int, P: int, seed: int = 0):
    """(logits [B, P], targets [B, P]) f32: N(0, 3) logits and grey targets, with
    +-PLANTED logits under targets 0 and 1 at the head of row 0 and the tail of
    the last row (20 positions each; -0.0 is planted as such)."""
    g = gen(seed)
    t = 3.0 * torch.randn(B, P, generator=g)
    x = torch.rand(B, P, generator=g)
    vals = [s * v for v in PLANTED for s in (1.0, -1.0)]
    pt = torch.tensor([v for v in vals for _ in (0, 1)], dtype=torch.float32)
    px = torch.tensor([float(k) for _ in vals for k in (0, 1)], dtype=torch.float32)
    n = pt.numel()
    t[0, :n], x[0, :n] = pt, px
    t[B - 1, P - n:], x[B - 1, P - n:] = pt, px
    return t.contiguous(), x.contiguous()


def adam_inputs(total: int, seed: int = 0):
    """p, g, m, v (f32 [total]); every fifth gradient is ten times larger, so
    (g * grad_scale)^2 > 77 on plenty of elements; v >= 1e-3."""
    gn = gen(seed)
    p = torch.randn(total, generator=gn)
    g = 3.0 * torch.randn(total, generator=gn)
    g[::5] *= 10.0
    m = 0.1 * torch.randn(total, generator=gn)
    v = 0.1 * torch.rand(total, generator=gn) + 1e-3
    return p, g, m, v


# lr, betas, eps, weight_decay, grad_scale, decoupled_wd, schedule fields (hpo/schedule.py)
ADAM_SETS = {
    "default": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, decoupled=False,
                    lr_warmup_steps=0),
    "coupled": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=0.5, decoupled=False,
                    lr_warmup_steps=0),
    "decoupled": dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, decoupled=True,
                      lr_warmup_steps=4000),
}


def f32(v) -> float:
    return float(np.float32(v))


def adam_consts(hp: dict, step: int, omb=None) -> dict:
    """What adam_consts_block computes for ``step`` (1-based t) from the HParams /
    TrainState images TrialState.set_hparams / set_step write. ``omb`` = (omb1,
    omb2) overrides the conv kernels' float32(1) - float32(beta)."""
    from multidisttorch_amd.hpo.schedule import Schedule

    lr_t = hp["lr"] * Schedule(lr_warmup_steps=hp.get("lr_warmup_steps", 0)).lr_factor(step)
    b1, b2 = f32(hp["beta1"]), f32(hp["beta2"])
    bc1 = 1.0 - math.pow(hp["beta1"], step)
    bc2 = 1.0 - math.pow(hp["beta2"], step)
    if omb is None:
        omb = (f32(np.float32(1) - np.float32(b1)), f32(np.float32(1) - np.float32(b2)))
    return dict(step_size=lr_t / bc1, bc2s=math.sqrt(bc2), b1=b1, b2=b2, eps=f32(hp["eps"]),
                wd=f32(hp["weight_decay"]), gs=f32(hp["grad_scale"]), lr=lr_t, decoupled=bool(hp["decoupled"]),
                omb1=omb[0], omb2=omb[1])


# ----------------------------------------------------------------- oracles ----
def reparam_ref(mulv, eps, beta: float = 1.0):
    """float64 (z, k, beta k) and the bounds (b_z, b_k) of z and of the
    per-element KLD term k = -0.5 (1 + lv - mu^2 - exp(lv)); the kernels'
    kld_part is the unweighted block sum of k, ``beta k`` what the loss adds."""
    Z = mulv.shape[-1] // 2
    mu, lv, e = mulv[..., :Z].double(), mulv[..., Z:].double(), eps.double()
    sd = torch.exp(0.5 * lv)
    z = mu + e * sd
    k = -0.5 * (1 + lv - mu * mu - sd * sd)
    b_z = 8 * U * (mu.abs() + (e * sd).abs())
    b_k = 0.5 * 8 * U * (1 + lv.abs() + mu * mu + sd * sd)
    return z, k, beta * k, b_z, b_k


def block_sum_ref(v, b_v, owners):
    """Per-block float64 sums of lane values ``v`` (any shape, flattened) with
    lane bounds ``b_v``, and their bounds."""
    v, b_v = v.reshape(-1).double(), b_v.reshape(-1).double()
    ref = torch.stack([v[o].sum() for o in owners])
    bound = torch.stack([b_v[o].sum() + (LANES + 4) * U * v[o].abs().sum() for o in owners])
    return ref, bound


def reparam_bwd_ref(dz, mulv, eps, beta: float, b_dz=None):
    """float64 d[mu|lv] [.., 2Z] of ``sum(g z) + beta KLD`` with g = dz, and its
    bound; ``b_dz``: the bound dz itself carries (a split-K sum) or None."""
    Z = mulv.shape[-1] // 2
    mu, lv, e, g = mulv[..., :Z].double(), mulv[..., Z:].double(), eps.double(), dz.double()
    sd = torch.exp(0.5 * lv)
    es = e * sd
    dm = g + beta * mu
    dl = 0.5 * g * es + 0.5 * beta * (sd * sd - 1)
    b_dm = 8 * U * (g.abs() + (beta * mu).abs())
    b_dl = 8 * U * ((0.5 * g * es).abs() + 0.5 * abs(beta) * (sd * sd + 1))
    if b_dz is not None:
        b_dm = b_dm + b_dz
        b_dl = b_dl + 0.5 * es.abs() * b_dz
    return torch.cat([dm, dl], -1), torch.cat([b_dm, b_dl], -1)


def bce_ref(t, x):
    """The project's logit-form BCE with the 100 clamp, p = sigmoid(t), g = p - x
    (float64) and their bounds: dict(loss, p, g, b_loss, b_p, b_g)."""
    t, x = t.double(), x.double()
    sp = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))   # softplus(t)
    loss = x * torch.clamp(sp - t, max=100.0) + (1 - x) * torch.clamp(sp, max=100.0)
    p = torch.sigmoid(t)
    g = p - x
    return dict(loss=loss, p=p, g=g, b_loss=8 * U * (x * (sp + t.abs()) + (1 - x) * sp) + TINY, b_p=8 * U * p + TINY,
                b_g=8 * U * (p + x.abs()) + TINY)


def bf16_bound(ref, b32):
    """Bound of a bf16 store with no f32 twin: one bf16 rounding of the f32
    value, which lies within ``b32`` of ``ref``."""
    return (1 + BF16_U) * b32 + BF16_U * ref.abs() + TINY


def slab_sum_ref(slab, bias=None):
    """float64 ``slab.sum(0) (+ bias)`` and its any-order f32 bound."""
    ks = slab.shape[0]
    s = slab.double()
    ref, mag = s.sum(0), s.abs().sum(0)
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    return ref, (ks + 4) * U * mag


def adam_ref(p, g, m, v, c: dict):
    """One Adam step in float64 with the constants ``c`` (adam_consts): the
    arithmetic of models.mlp_vae.reference_adam_ (torch.optim.Adam / AdamW)
    with the two moment weights taken from ``c``. Returns (p, m, v, b_p, b_m, b_v)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gr = g * c["gs"]
    mag = gr.abs()
    b_p1 = torch.zeros_like(p)
    if c["wd"] != 0:
        if c["decoupled"]:
            b_p1 = 4 * U * p.abs()
            p = p * (1 - c["lr"] * c["wd"])
        else:
            mag = mag + (c["wd"] * p).abs()
            gr = gr + c["wd"] * p
    b_gr = 2 * U * mag
    m2 = m + c["omb1"] * (gr - m)                      # exp_avg.lerp_(gr, 1 - beta1)
    b_m = U * (m2.abs() + c["omb1"] * (gr.abs() + m.abs())) + c["omb1"] * b_gr
    v2 = c["b2"] * v + c["omb2"] * gr * gr            # exp_avg_sq.mul_(beta2).addcmul_(gr, gr, 1 - beta2)
    b_v = U * (v2 + c["omb2"] * gr * gr + c["b2"] * v) + 2 * c["omb2"] * gr.abs() * b_gr
    s = v2.sqrt()
    q = s / c["bc2s"]
    den = q + c["eps"]
    b_den = 8 * U * q + torch.where(s > 0, b_v / (2 * s * c["bc2s"]).clamp_min(1e-300), torch.zeros_like(s)) + U * den
    upd = c["step_size"] * m2 / den
    p2 = p - upd
    b_p = b_p1 + U * p2.abs() + upd.abs() * (7 * U + b_den / den) + c["step_size"] * b_m / den
    return p2, m2, v2, b_p, b_m, b_v


def eps_ratio(got, B: int, Z: int, seed: int, stream: int, state_step: int) -> float:
    """Philox noise of a kernel handed a state at ``state_step``: the counter
    is keyed with ``state_step - 1`` (the running step's 0-based index)."""
    from multidisttorch_amd.ops.philox import reparam_eps

    want = torch.from_numpy(reparam_eps(B, Z, seed, stream, state_step - 1).astype(np.float64))
    err = (got.double().reshape(B, Z) - want).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    return float((err / (EPS_TOL + EPS_TOL * want.abs())).max())


__all__ = ["U", "ratio", "TINY", "BF16_U", "BF16_FILL", "splitk_rp", "rows_ok", "row_ks", "block_owners",
           "reparam_inputs", "slab_inputs", "bce_inputs", "adam_inputs", "ADAM_SETS", "adam_consts", "reparam_ref",
           "block_sum_ref", "reparam_bwd_ref", "bce_ref", "bf16_bound", "slab_sum_ref", "adam_ref", "eps_ratio"]
