"""Checker of the conv GEMM tile tests (igemm_fwd_k, wgrad_k and the split-K
combine of csrc/kernels/conv_igemm_dev.h): float64 oracles, one derived
per-element bound, sentinel buffers. Used by tests/unit/test_igemm_checker.py
(CPU: the checker is not vacuous) and tests/gpu/test_conv_igemm_tiles.py.

Inputs are bf16 (an f32 A or X is rounded to bf16 by the oracle exactly as the
kernel's gather rounds it, to nearest even), so every product a * w has at most
16 significand bits and is EXACT in f32: the kernels' only error is the f32
summation. With ``mag`` the same operation on |a|, |w|, |bias|:

    |y32 - ref| <= (K + 9) 2^-23 mag                 one launch, K products per output
    |y32 - ref| <= (K + ksplit + 9) 2^-23 mag        split-K, after the combine
    |z_s - ref_s| <= (K_s + 9) 2^-23 mag_s           raw split-K slab s (its K_s products)

Derivation: K exact products are added in an order the test does not fix (MFMA
lanes, k-halves, k-tiles). Each addition rounds its partial sum with relative
error at most 2^-23, which covers round-to-nearest (2^-24) as well as a
truncating MFMA accumulator; n additions in any order give at most
n 2^-23 sum|terms| to first order (Higham, Accuracy and Stability, section 4.2).
The extra 9 covers the bias add, the exchange between k-halves (KWS == 2) and
the second-order terms; the combine adds ksplit slab values. ReLU and the
output mask are 1-Lipschitz or exact, so they do not enlarge the bound. No
tolerance of this module is measured, and every element is compared.

* bf16 twin: y16 and y32 are stored from the same register, so
  ``y16 == y32.bfloat16()`` bit for bit.
* Weight gradient: m-split s sums rows [64 mps s, 64 mps (s + 1)) of the
  G^T im2col(X) product: slab s within (rows_s + 9) 2^-23 mag_s of its float64
  value, and the float64 sum of the slabs within the sum of those bounds of
  the full gradient.
* Column sums: partial row (class, m-tile) is the f32 sum of the BM values the
  same launch stored to y32 (after ReLU and mask): within
  (BM + 9) 2^-23 sum|v| of the float64 sum of those y32 rows. Parity-mode rows
  are mapped to pixels here (``parity_rows``), not by the kernel's arithmetic.
* Sentinels: every output is allocated GUARD elements longer than the plan
  says is written and pre-filled (NaN for f32, BF16_FILL for bf16); afterwards
  the in-range part is finite and the guard bit-identical to its fill.

All results are error/bound ratios (``mlp_checker.ratio``): pass means <= 1.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from multidisttorch_amd.ops.conv_layout import parity_transpose
from tests import igemm_cases as cs
from tests.mlp_checker import ratio

EPS = 2.0 ** -23      # relative error of one f32 addition, rounding to nearest or truncating
SLACK = 9             # bias add, k-half exchange, second-order terms
GUARD = 4096          # sentinel elements past every output
BF16_FILL = 24576.0   # bf16 poison: exactly representable, far outside what the cases produce
BF = torch.bfloat16
F64 = torch.float64


# ------------------------------------------------------------------ inputs ----
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def fwd_inputs(mode, shape, a_f32=False, seed=0, device="cpu"):
    """Operands of a forward-type GEMM in conv view: A (NHWC conv input in conv
    mode, NHWC conv output in parity mode; bf16, or f32 in [0, 1) for
    ``a_f32``), w [CO, k, k, C] bf16, B16 (what the kernel reads: w flat, or its
    parity-ordered transpose), bias [Ncols] f32 and a bf16 output mask of both
    signs with exact zeros, in the output's NHWC order."""
    N, H, C, CO, k, s, p = shape
    OH = cs.desc(shape)[4]
    classes, M, Ncols, K = cs.fwd_geom(mode, shape)
    g = _gen(seed, device)
    ashape = (N, H, H, C) if mode == cs.CONV else (N, OH, OH, CO)
    if a_f32:
        A = torch.rand(ashape, generator=g, device=device)
    else:
        A = torch.randn(ashape, generator=g, device=device).to(BF)
    w = (torch.randn((CO, k, k, C), generator=g, device=device) / K ** 0.5).to(BF)
    bias = torch.randn((Ncols,), generator=g, device=device)
    rows = classes * M
    mask = torch.randn((rows, Ncols), generator=g, device=device)
    zero = torch.rand((rows, Ncols), generator=g, device=device) < 0.125
    mask = torch.where(zero, torch.zeros_like(mask), mask).to(BF)
    B16 = w.flatten() if mode == cs.CONV else parity_transpose(w, s)
    return dict(A=A, w=w, B16=B16.contiguous(), bias=bias, mask=mask)


def wgrad_inputs(shape, x_f32=False, seed=0, device="cpu"):
    """X (NHWC conv input, bf16 or f32 in [0, 1)) and G (NHWC output gradient, bf16)."""
    N, H, C, CO, k, s, p = shape
    OH = cs.desc(shape)[4]
    g = _gen(seed, device)
    X = torch.rand((N, H, H, C), generator=g, device=device)
    X = X if x_f32 else (2 * X - 1).to(BF)
    G = torch.randn((N, OH, OH, CO), generator=g, device=device).to(BF)
    return dict(X=X, G=G)


# ----------------------------------------------------------------- oracles ----
def as64(t):
    """float64 of a kernel operand: an f32 operand rounds to bf16 first."""
    return t.to(BF).to(F64)


def im2col(x, k, s, p):
    """[N, H, W, C] -> [N OH OW, k k C], columns ordered (ky, kx, c), zero padding."""
    N, H, W, C = x.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = F.pad(x, (0, 0, p, p, p, p))
    taps = [xp[:, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s, :] for ky in range(k) for kx in range(k)]
    return torch.stack(taps, 3).reshape(N * OH * OW, k * k * C)


def conv_ref(x, w, s, p, k_lo=0, k_hi=None):
    """float64 conv of NHWC x with w [CO, k, k, C] over the products k_lo <= (ky, kx, c) < k_hi:
    [N OH OW, CO]."""
    CO, k = w.shape[0], w.shape[1]
    cols, wm = im2col(x, k, s, p), w.reshape(CO, -1)
    return cols[:, k_lo:k_hi] @ wm[:, k_lo:k_hi].T


def tconv_ref(g, w, s, p, H):
    """float64 transposed conv (the conv's backward-data) of NHWC g [N, OH, OW, CO]
    with w [CO, k, k, C], by its definition: tap (ky, kx) of output pixel
    (oy, ox) lands on input pixel (s oy + ky - p, s ox + kx - p). [N H H, C]."""
    N, OH, OW, CO = g.shape
    k, C = w.shape[1], w.shape[3]
    full = torch.zeros((N, s * (OH - 1) + k, s * (OW - 1) + k, C), dtype=g.dtype, device=g.device)
    gm = g.reshape(-1, CO)
    for ky in range(k):
        for kx in range(k):
            tap = (gm @ w[:, ky, kx, :]).view(N, OH, OW, C)
            full[:, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s, :] += tap
    assert full.shape[1] >= p + H
    return full[:, p:p + H, p:p + H, :].reshape(N * H * H, C)


def fwd_acc(mode, shape, inp):
    """(acc, mag) [rows, Ncols] float64 in the output's NHWC order: the bare
    sum of products and the same sum of their magnitudes. Computed once per
    case; ``epilogue`` leaves both unchanged."""
    N, H, C, CO, k, s, p = shape
    a, w = as64(inp["A"]), inp["w"].to(F64)
    if mode == cs.CONV:
        return conv_ref(a, w, s, p), conv_ref(a.abs(), w.abs(), s, p)
    return tconv_ref(a, w, s, p, H), tconv_ref(a.abs(), w.abs(), s, p, H)


def fwd_ref(mode, shape, inp, bias=False, relu=False, mask=False):
    """(ref, mag) [rows, Ncols] float64 with the epilogue the call uses."""
    return epilogue(*fwd_acc(mode, shape, inp), inp, bias, relu, mask)


def epilogue(ref, mag, inp, bias=False, relu=False, mask=False):
    if bias:
        b = inp["bias"].to(F64)
        ref, mag = ref + b, mag + b.abs()
    if relu:
        ref = torch.relu(ref)
    if mask:
        ref = torch.where(inp["mask"].to(F64) > 0, ref, torch.zeros_like(ref))
    return ref, mag


def fwd_bound(mag, K, ksplit=1):
    return (K + (ksplit if ksplit > 1 else 0) + SLACK) * EPS * mag


def check_fwd(y32, ref, mag, K, ksplit=1) -> float:
    return ratio(y32.reshape(ref.shape), ref, fwd_bound(mag, K, ksplit))


def twin_ok(y16, y32) -> bool:
    """y16 is the bf16 rounding of the very value stored to y32."""
    return torch.equal(y16.view(torch.int16), y32.to(BF).view(torch.int16))


def slab_refs(shape, inp, ktiles, kt_per_split):
    """Per split-K slab of a conv-mode call: (ref_s, bound_s), the float64 sum
    over k-tiles [s kps, (s + 1) kps) and its bound."""
    N, H, C, CO, k, s, p = shape
    a, w = as64(inp["A"]), inp["w"].to(F64)
    K = k * k * C
    out = []
    for kt0 in range(0, ktiles, kt_per_split):
        lo, hi = 64 * kt0, min(K, 64 * (kt0 + kt_per_split))
        ref, mag = conv_ref(a, w, s, p, lo, hi), conv_ref(a.abs(), w.abs(), s, p, lo, hi)
        out.append((ref, (hi - lo + SLACK) * EPS * mag))
    return out


# ------------------------------------------------------------ parity rows ----
def parity_rows(shape, cls, device="cpu"):
    """Flat NHWC pixel index (n H + iy) W + ix of every row of parity class
    ``cls`` = ca S + cb: row m = (n, yy, xx) is pixel (n, S yy + oa, S xx + ob)
    with oa = (ca - P) mod S, ob = (cb - P) mod S."""
    N, H, C, CO, k, s, p = shape
    ca, cb = divmod(cls, s)
    oa, ob = (ca - p) % s, (cb - p) % s
    n = torch.arange(N, device=device).view(N, 1, 1)
    iy = (s * torch.arange(H // s, device=device) + oa).view(1, -1, 1)
    ix = (s * torch.arange(H // s, device=device) + ob).view(1, 1, -1)
    return ((n * H + iy) * H + ix).reshape(-1)


def class_rows(mode, shape, device="cpu"):
    """Per class, the flat output row of every GEMM row."""
    classes, M, _, _ = cs.fwd_geom(mode, shape)
    if mode == cs.CONV:
        return [torch.arange(M, device=device)]
    return [parity_rows(shape, c, device) for c in range(classes)]


def colsum_ref(y32, mode, shape, BM):
    """(ref, bound) [classes mtiles, Ncols]: float64 sums of the y32 rows of each
    (class, m-tile) and their bounds."""
    classes, M, Ncols, _ = cs.fwd_geom(mode, shape)
    mtiles = -(-M // BM)
    y = y32.reshape(-1, Ncols).to(F64)
    ref, mag = [], []
    for rows in class_rows(mode, shape, y.device):
        v = torch.zeros((mtiles * BM, Ncols), dtype=F64, device=y.device)
        v[:M] = y[rows]
        v = v.view(mtiles, BM, Ncols)
        ref.append(v.sum(1))
        mag.append(v.abs().sum(1))
    return torch.cat(ref), (BM + SLACK) * EPS * torch.cat(mag)


# --------------------------------------------------------- weight gradient ----
def wgrad_ref(shape, inp, mt_per_split):
    """(slabs, full): per m-split (ref_s, bound_s) [CO, K2] of the rows
    [64 mps s, 64 mps (s + 1)), and the full float64 gradient [CO, K2] (columns
    ordered (ky, kx, c), the layout of w)."""
    N, H, C, CO, k, s, p = shape
    cols = im2col(as64(inp["X"]), k, s, p)
    G = inp["G"].to(F64).reshape(-1, CO)
    M = G.shape[0]
    step = 64 * mt_per_split
    slabs = []
    for r0 in range(0, M, step):
        g, c = G[r0:r0 + step], cols[r0:r0 + step]
        slabs.append((g.T @ c, (g.shape[0] + SLACK) * EPS * (g.abs().T @ c.abs())))
    return slabs, G.T @ cols


def check_wgrad(out, shape, inp, nsplit, mt_per_split):
    """(worst slab ratio, ratio of the float64 slab sum against the full gradient)."""
    N, H, C, CO, k, s, p = shape
    numel = CO * k * k * C
    slabs, full = wgrad_ref(shape, inp, mt_per_split)
    assert len(slabs) == nsplit, (len(slabs), nsplit)
    got = out[:nsplit * numel].view(nsplit, CO, k * k * C)
    worst = max(ratio(got[i], ref, b) for i, (ref, b) in enumerate(slabs))
    total = ratio(got.to(F64).sum(0), full, sum(b for _, b in slabs))
    return worst, total


# ---------------------------------------------------------------- sentinels ----
def _fill(dtype):
    return float("nan") if dtype == torch.float32 else BF16_FILL


def guarded(n, dtype=torch.float32, device="cpu"):
    """A buffer of n + GUARD elements, all poison."""
    return torch.full((n + GUARD,), _fill(dtype), dtype=dtype, device=device)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b) -> bool:
    """Two buffers, guards included, hold the same bits (NaN poison compares equal)."""
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def untouched(t, start=0) -> bool:
    """t[start:] is bit-identical to its fill."""
    tail = t[start:]
    return torch.equal(_bits(tail), _bits(torch.full_like(tail, _fill(t.dtype))))


def written(t, n) -> bool:
    """The first n elements were all written with finite values and the guard
    behind them is intact."""
    ok = bool(torch.isfinite(t[:n].float()).all())
    if t.dtype != torch.float32:
        ok = ok and not bool((t[:n].float() == BF16_FILL).any())
    return ok and untouched(t, n)
