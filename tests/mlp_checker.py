"""Shared checker of the MLP-VAE kernel tests (tests/unit/test_mlp_checker.py,
tests/gpu/test_mlp_vae_shapes.py): the swept shapes and a stage-wise comparison
whose bounds are derived, not measured.

Let u = 2^-24 (f32 unit roundoff).

* GEMM stage ``C = A B (+ bias)`` with reduction length K: the reference is the
  float64 product of the operands the kernel consumed (read back from the
  device), and every element must satisfy
  ``|got - ref| <= (K + 4) u (|A| |B| + |bias|)``: the textbook worst case of an
  f32 dot product of length K in any summation order (Higham, Accuracy and
  Stability of Numerical Algorithms, section 3.1), plus the epilogue's few
  roundings. ReLU, and a ReLU mask taken from a stored (separately checked)
  activation, are 1-Lipschitz and keep the bound.
* Elementwise stages (z, recon = sigmoid(t), dlog = p - x, dmu, dlv): the feeding
  GEMM's bound through the formula's partial derivatives (sigmoid: |dp| <= |dt|/4)
  plus ``8 u sum|terms|`` for the formula's own roundings.
* Philox noise: ``ops.philox.reparam_eps`` at rtol = atol = 1e-5.
* Free bits (``fb`` > 0): the floored set is the float64 one, kl_d < fb, from the
  stored mulv (the tests keep every element away from the floor:
  ``free_bits_cases.check_floor``); a floored element adds exactly fb to the KLD
  sum and its KL gradient is exactly zero (weight 0 in the dmu / dlv formulas).
* Total-correlation penalty (``tc`` = (tc_t, g64, bg) of ``knob_cases.tc_of``):
  d[mu|lv] is the value and bound above plus ``tc_t g64`` within
  ``tc_t bg + 2 u max(|before|, |after|)`` (``knob_cases.tc_rule``); the later
  stages (dh1, the fc21 / fc22 gradients) read the stored dmulv and so show that
  their kernels consumed the folded value.
* Loss: relative 1e-4. The BCE terms are non-negative and no value passes
  through more than a few hundred additions (F3's tile and wave sums, then at
  most 256 partials per thread in the loss reduction at the last BCE slot), so
  the summation error stays below ~400 u = 2.4e-5 relative at every shape.

All results are error/bound ratios: a stage passes when its ratio is <= 1.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

U = 2.0 ** -24
LOSS_REL = 1e-4

# The smallest shapes that reach each path of csrc/kernels/vae_mlp.hip (B, rows M
# per case, D, H, Z). th = ceil(H/16) slab slices, groups = ceil(th/8),
# ntm = ceil(2Z/16), ntz = ceil(Z/16).
SHAPES = {
    # the checker itself at the one point every earlier test covers (th = 25, groups = 4, ntm = 3, ntz = 2)
    "default": dict(B=128, Ms=(128, 37), D=784, H=400, Z=20),
    # one partial tile per dimension; D = 20 is 2 k-chunks, so 6 of F1/B1's 8 waves (and at M = 5 one of the
    # weight-gradient waves) get an empty k range; th = 2 < 8: one group; ntm = ntz = 1
    "tiny": dict(B=16, Ms=(16, 5), D=20, H=20, Z=4),
    # th = 8 > D/4 = 5: the xb copy split leaves three of a row tile's blocks no column quad
    "xbsplit": dict(B=16, Ms=(16,), D=20, H=128, Z=4),
    # no dimension a multiple of 16: every min(k0, K-4) clamp and 0/1 tail mask on D and H fires
    # (ARowMajor, ARowGather, BWeightNT, the raw prefetches of F1/F2/B1/B2); partial second [mu|lv] tile (2Z = 24)
    "ragged": dict(B=48, Ms=(48, 37), D=100, H=36, Z=12),
    # th = 32 (both half sums and all four quarter sums full), groups = 4, ntm = 4, ntz = 2 full: the LDS tiles
    # zt[16][36], dml[16][68], part[2][16][64] at full width; second k round in F3 / dec2 (K = 512 > 448)
    "wide": dict(B=32, Ms=(32, 17), D=256, H=512, Z=32),
    # D = 1156: 73 k-chunks, two rounds of wave_tile<7> in F1/B1 with a ragged second round; ntm = 2
    "d2": dict(B=32, Ms=(32,), D=1156, H=64, Z=8),
    # the --image-size 128 shape: 1024 chunks, 19 rounds per wave
    "img128": dict(B=16, Ms=(16, 9), D=16384, H=400, Z=20),
    # K = M > 128: two weight-gradient rounds per wave (16 pairs each), ragged at M = 200
    "brounds": dict(B=256, Ms=(256, 200), D=784, H=400, Z=20),
    # B not a multiple of 16 (Bpad rows in the slabs)
    "b200": dict(B=200, Ms=(200,), D=784, H=400, Z=20),
    # the last KLD partial slot (256 row tiles * 8); 32 weight-gradient rounds
    "bmax": dict(B=4096, Ms=(4096, 4081), D=32, H=32, Z=4),
    # the last BCE partial slot (8192 F3 blocks * 8); forward and loss only
    "bce_full": dict(B=256, Ms=(256,), D=16384, H=400, Z=20, forward_only=True),
}

# GEMMs whose dropped k-chunk / row pair the bound cannot see reliably (long
# reductions: the mutant's error is of the size of the bound) are covered by the
# exact-arithmetic tests of tests/gpu/test_mlp_vae_shapes.py instead, at these
# reduction lengths: F1/B1 with K = D, the weight gradients with K = M.
EXACT_D = {1156: "d2", 16384: "img128"}
EXACT_M = {200: "brounds", 256: "brounds", 4081: "bmax", 4096: "bmax"}


def cases(ids=None, forward_only=None):
    """[(id, M)] over the table (optionally a subset of ids)."""
    out = []
    for k, s in SHAPES.items():
        if ids is not None and k not in ids:
            continue
        if forward_only is not None and bool(s.get("forward_only")) != forward_only:
            continue
        out += [(k, m) for m in s["Ms"]]
    return out


# ------------------------------------------------------------------ bounds ----
def gemm_ref(A, B, bias=None):
    """float64 ``A @ B (+ bias)`` and its per-element bound."""
    A, B = A.double(), B.double()
    K = A.shape[1]
    ref = A @ B
    mag = A.abs() @ B.abs()
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    return ref, (K + 4) * U * mag


def ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; an error where the bound is 0 counts as inf."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    zero = bound <= 0
    if bool((err[zero] > 0).any()):
        return math.inf
    r = err[~zero] / bound[~zero]
    return float(r.max()) if r.numel() else 0.0


def outside(got, ref, bound) -> float:
    """Fraction of elements outside the bound."""
    return float(((got.double() - ref).abs() > bound).double().mean())


def check_gemm(got, A, B, bias=None, relu=False, mask=None) -> float:
    ref, bound = gemm_ref(A, B, bias)
    if relu:
        ref = torch.relu(ref)
    if mask is not None:
        ref = ref * mask.to(ref.dtype)
        bound = bound * mask.to(ref.dtype)
    return ratio(got, ref, bound)


def _w(v):
    d = {k: t.double() for k, t in v.items()}
    return (d["fc1.weight"], d["fc1.bias"], torch.cat([d["fc21.weight"], d["fc22.weight"]], 0),
            torch.cat([d["fc21.bias"], d["fc22.bias"]], 0), d["fc3.weight"], d["fc3.bias"], d["fc4.weight"],
            d["fc4.bias"])


def bce_terms(t, x):
    sp_pos = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    return x * torch.clamp(sp_pos - t, max=100.0) + (1 - x) * torch.clamp(sp_pos, max=100.0)


def floored_set(mulv, Z: int, fb: float):
    """The float64 floored set kl_d < fb ([M, Z] bool; empty for fb = 0)."""
    m = mulv.double()
    mu, lv = m[:, :Z], m[:, Z:]
    kl = 0.5 * (mu * mu + torch.exp(lv) - 1 - lv)
    return kl < fb if fb > 0 else torch.zeros_like(kl, dtype=torch.bool)


def check_forward(dev: Dict[str, torch.Tensor], v, x, beta: float, eps_host: Optional[np.ndarray],
                  loss: Optional[float], fb: float = 0.0) -> Dict[str, float]:
    """Ratios of the stored forward stages. ``dev``: CPU copies of the device's
    h1, mulv, eps, z, h3 and (when stored) recon, dlog; ``v``: parameter views;
    ``x``: the batch rows; ``loss``: the device's loss (None: not checked)."""
    W1, b1, W2, b2, W3, b3, W4, b4 = _w(v)
    x = x.double()
    Z = W3.shape[1]
    d = {k: t.double() for k, t in dev.items()}
    out = {}
    out["h1"] = check_gemm(d["h1"], x, W1.t(), b1, relu=True)
    out["mulv"] = check_gemm(d["mulv"], d["h1"], W2.t(), b2)
    if eps_host is not None:
        e = (d["eps"] - torch.from_numpy(np.asarray(eps_host, dtype=np.float64))).abs()
        out["eps"] = float((e / (1e-5 + 1e-5 * d["eps"].abs())).max())
    mu, lv = d["mulv"][:, :Z], d["mulv"][:, Z:]
    sd = torch.exp(0.5 * lv)
    out["z"] = ratio(d["z"], mu + d["eps"] * sd, 8 * U * (mu.abs() + (d["eps"] * sd).abs()))
    out["h3"] = check_gemm(d["h3"], d["z"], W3.t(), b3, relu=True)
    t, bt = gemm_ref(d["h3"], W4.t(), b4)
    p = torch.sigmoid(t)
    if "recon" in d:
        out["recon"] = ratio(d["recon"], p, bt / 4 + 8 * U * p)
    if "dlog" in d:
        out["dlog"] = ratio(d["dlog"], p - x, bt / 4 + 8 * U * (p + x.abs()))
    if loss is not None:
        kl = -0.5 * (1 + lv - mu * mu - sd * sd)
        kld = torch.where(floored_set(d["mulv"], Z, fb), torch.full_like(kl, fb), kl).sum()
        ref = float(bce_terms(t, x).sum() + beta * kld)
        out["loss"] = abs(loss - ref) / (LOSS_REL * abs(ref))
    return out


def dmulv_ref(d, W3, beta: float, fb: float = 0.0, tc=None):
    """(ref, bound) of d[mu|lv] from the stored dh3, mulv and eps (float64 dict ``d``)."""
    from tests.knob_cases import tc_rule

    Z = W3.shape[1]
    dz, bz = gemm_ref(d["dh3"], W3)
    mu, lv = d["mulv"][:, :Z], d["mulv"][:, Z:]
    sd = torch.exp(0.5 * lv)
    es = d["eps"] * sd
    # beta: the KL weight, or an [M, Z] tensor of per-element weights (tests/gpu/test_free_bits_gpu.py)
    bt = beta.double() if torch.is_tensor(beta) else torch.full_like(mu, beta)
    be = torch.where(floored_set(d["mulv"], Z, fb), torch.zeros_like(mu), bt)
    dmu = dz + be * mu
    bmu = bz + 8 * U * (dz.abs() + (be * mu).abs())
    dlv = 0.5 * dz * es + 0.5 * be * (sd * sd - 1)
    blv = bz * 0.5 * es.abs() + 8 * U * ((0.5 * dz * es).abs() + 0.5 * be.abs() * (sd * sd + 1))
    return tc_rule(torch.cat([dmu, dlv], 1), torch.cat([bmu, blv], 1), tc)


def check_backward(dev: Dict[str, torch.Tensor], grads, v, x, beta: float, fb: float = 0.0,
                   tc=None) -> Dict[str, float]:
    """Ratios of the stored backward stages and the ten gradient tensors, each
    against float64 from the device's own inputs of that stage. ``fb``: the
    floor the kernels read; ``tc``: (tc_t, g64, bg) or None (module docstring)."""
    W1, b1, W2, b2, W3, b3, W4, b4 = _w(v)
    x = x.double()
    d = {k: t.double() for k, t in dev.items()}
    g = {k: t.double() for k, t in grads.items()}
    M = x.shape[0]
    ones = torch.ones(M, 1, dtype=torch.float64)
    out = {}
    m3, m1 = d["h3"] > 0, d["h1"] > 0
    out["dh3"] = check_gemm(d["dh3"], d["dlog"], W4, mask=m3)
    out["dmulv"] = ratio(d["dmulv"], *dmulv_ref(d, W3, beta, fb, tc))
    out["dh1"] = check_gemm(d["dh1"], d["dmulv"], W2, mask=m1)

    def wg(name_w, name_b, dy, a):  # dW = dy^T a, db = dy^T 1 (K = M)
        gw = torch.cat([g[n] for n in name_w], 0)
        gb = torch.cat([g[n] for n in name_b], 0)
        out["g" + name_w[0].split(".")[0]] = max(check_gemm(gw, dy.t(), a), check_gemm(gb[:, None], dy.t(), ones))

    wg(["fc4.weight"], ["fc4.bias"], d["dlog"], d["h3"])
    wg(["fc3.weight"], ["fc3.bias"], d["dh3"], d["z"])
    wg(["fc21.weight", "fc22.weight"], ["fc21.bias", "fc22.bias"], d["dmulv"], d["h1"])
    wg(["fc1.weight"], ["fc1.bias"], d["dh1"], x)
    return out


# ---------------------------------------------------- exact-arithmetic data ----
def exact_ok(A, B, bias=None, lsb: float = 1.0) -> bool:
    """The two host checks of an exact test: the float64 result is an f32 number,
    and sum|a||b| (+ |bias|), counted in units of the result's least significant
    bit ``lsb``, stays below 2^24, so every partial sum in any order is exact."""
    ref, _ = gemm_ref(A, B, bias)
    mag = A.double().abs() @ B.double().abs()
    if bias is not None:
        mag = mag + bias.double().abs()
    return bool((ref.float().double() == ref).all()) and float(mag.max()) / lsb < 2.0 ** 24


def randint(g, shape, lo, hi):
    """Integers in [lo, hi] as float32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# stage names in step order (the keys of check_forward + check_backward; AD and EM: tests/knob_cases.py)
STAGES = ("h1", "mulv", "eps", "z", "h3", "recon", "dlog", "loss", "dh3", "dmulv", "dh1", "gfc4", "gfc3", "gfc21",
          "gfc1", "AD", "EM")


def first_failure(ratios: dict):
    """The first stage (in step order) with a ratio > 1, or None."""
    for st in STAGES:
        if any(not r <= 1 for k, r in ratios.items() if k.split(".")[0] == st):
            return st
    return None
