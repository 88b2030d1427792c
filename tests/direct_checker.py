"""Checker of the direct and single-channel conv kernel tests (conv_direct.h,
conv_dwgrad.h, conv_thin.h, conv_thin_wg.h): float64 oracles, derived
per-element bounds, exact-data generators and the row / block maps of every
partial output. Used by tests/unit/test_direct_checker.py (CPU: the checker
passes an f32 emulation and fails each mutated one) and
tests/gpu/test_conv_direct_domain.py (the kernels). It extends
tests/igemm_checker.py (``ck``): the same sentinels, the same error/bound
ratios (pass means <= 1), and NO tolerance measured on a kernel.

Notation: EPS = 2^-23 bounds one f32 addition inside an MFMA accumulator
(rounding to nearest or truncating), U = 2^-24 one correctly rounded VALU
operation (fmaf, add), SLACK = 9 covers the bias add, exchanges between wave
groups and second-order terms; ``mag`` is the same operation on the absolute
values of the operands as the kernel reads them. n exact products added in any
order carry at most n * (EPS | U) * mag (Higham, section 4.2).

Direct conv (dconv_body). Operands are bf16, so every product is exact in f32
and ``ck.check_fwd`` applies unchanged: |y32 - ref| <= (K + SLACK) EPS mag with
K = 16 C (conv) or 4 CO (one parity class); the add of the second k-group's
accumulators (KS = 2: DcS3, DcT1) is one of the SLACK terms. y16 is stored from
the register y32 is stored from: ``ck.twin_ok``, bit for bit; a launch that
stores y16 alone must store the bits of the launch that stored both.
  Column sums: workgroup (n, rb) owns R output rows of image n in conv mode,
R class-grid rows of all four parity classes in transposed mode, i.e. the 2 R
output rows 2 R rb .. 2 R rb + 2 R - 1 (class (ca, cb) of grid row j holds
output row 2 j + (ca + 1) % 2). Either way row n RB + rb is the f32 sum of a
contiguous NHWC block of ``cnt`` pixels of the y32 the same launch stored:
|colsum - sum| <= (cnt + SLACK) EPS sum|v| (``direct_colsum_ref``).

Direct weight gradient (dwgrad_body): partial row n is the gradient of image n
alone, OH^2 exact bf16 products per element: ``ck.check_wgrad`` with one
"m-split" per image, |row_n - ref_n| <= (OH^2 + SLACK) EPS mag_n, and the
float64 sum of the rows against the full gradient under the sum of the bounds.

thin_wgrad_k (thin_wgrad_mfma_body): partial row (n, q) is the gradient of
output rows 4 q .. 4 q + 3 of image n, 256 pixels. bf16 X: 256 exact products,
(256 + SLACK) EPS mag. f32 X is split x = hi + lo + lo2 (three bf16 terms);
x - hi and x - hi - lo are exact in f32 and have at most 16 and 8 significant
bits, so the split has no residual for normal x (a 2^-24 |x| line is kept for
it); the code multiplies all three terms with g: 3 * 256 exact products whose
magnitudes sum to at most (1 + 2^-7) mag: (768 + SLACK) EPS (1 + 2^-7) mag +
2^-24 mag. The oracle takes an f32 X as it is (``thin_wgrad_refs``).

thin_conv / thin_tconv, VALU bodies: one fmaf chain per output, seeded with the
bias, over 16 taps or 4 CO (tap, channel) pairs, every operand read as stored
(f32 weights, f32 or bf16 input): (n + SLACK) U mag, n = 17 or 4 CO + 1.

thin_conv, MFMA body. With W = Wh + Wl + Wl2 and x = xh + xl + xl2 (bf16 terms,
|v - vh| <= 2^-8 |v|, |v - vh - vl| <= 2^-16 |v|, the three-term split exact as
above) the code computes (Wh + Wl + Wl2)(xh + xl) + Wh xl2 per tap:
  * dropped cross terms (Wl + Wl2) xl2: <= (2^-8 + 2^-16) 2^-16 |W||x| per tap
    <= 1.01 * 2^-24 mag per output (zero for bf16 input, where xl = xl2 = 0);
  * split residual: 0 for normal values; one 2^-24 mag line covers it;
  * accumulation: the MFMAs of the small terms run first; their <= 96 products
    sum to <= 3.1 * 2^-8 mag, so their roundings stay under 96 EPS 3.1 2^-8 mag
    < 1.2 EPS mag; the last MFMA adds the 32 products Wh xh, Wh xl to that
    accumulator: 33 additions on <= (1 + 2^-6) mag: < 34 EPS mag; the bias
    add is in SLACK.
  Total: (36 + SLACK) EPS mag + 2^-23 mag = (38 + SLACK) EPS mag.
thin_conv stores only y16: it is checked as the bf16 rounding of a value within
the bound of the oracle, |y16 - ref| <= bound + half a bf16 ulp of
|ref| + bound (``y16_ratio``). Its column-sum row b is the f32 sum of the
pre-rounding values of pixels 256 b .. 256 b + 255 (dead lanes of the tail
block add zero): the element bounds added plus (256 + SLACK) EPS sum|ref|.

thin_tconv, MFMA body: the bf16 activations are exact, the weights three exact
terms; every output adds 3 * 4 CO exact nonzero products (rows hi, lo, lo2 of
the A fragment; the other k positions multiply zero weights), then lo + lo2 +
hi and the bias: the hi row carries 4 CO EPS mag, the lo rows 2^-8 of that:
(4 CO + 3 + SLACK) EPS mag + 2^-24 mag for the residual line.

Fused BCE (all thin_tconv bodies): ``conv_small_checker.bce_ref`` at the
oracle's logit gives loss, p, g and the bounds of the formulas' own roundings;
the logit bound b_t enters through |d loss / d t| = |p - x| <= 1 and
|d p / d t| <= 1/4: b_loss + b_t, b_p + b_t / 4, b_g + b_t / 4; dlog16 adds one
bf16 rounding (``bf16_bound``). part[bid] / gpart[bid] are checked against the
float64 sum over exactly their block's pixels (``tconv_valu_owners``: block
class * gx + x holds class-grid pixels 256 x .. 256 x + 255 of its parity class;
``tconv_patch_owners``: block (n, q) holds output rows 8 q .. 8 q + 7 of image
n), bound = the pixel bounds added + (pixels + SLACK) U sum|v|.

Exact-data cases: inputs are small integers or multiples of 2^-20 chosen so
that the sum of the ABSOLUTE values of all terms of every output, column sum
and slab element stays below 2^24 units of the last place (``exact_fits``
checks this on the oracle's ``mag``). Every partial sum in any order is then
exactly representable, and the kernel's f32 results must equal the float64
oracle bit for bit. ``needs3`` data (19 significant bits: odd multiples of
2^-20 in [1/4, 1/2) whose residual after hi does not fit lo's 8 bits) makes
every bf16 term hi, lo, lo2 nonzero, so a dropped
term or one landing in the wrong k-half changes bits.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import direct_cases as dc
from tests import igemm_checker as ck
from tests.conv_small_checker import TINY, bce_ref, bf16_bound
from tests.igemm_checker import (BF, EPS, F64, SLACK, epilogue, fwd_acc, guarded, same_bits, twin_ok,  # noqa: F401
                                 untouched, written)
from tests.mlp_checker import U, ratio  # noqa: F401

UNIT = 2.0 ** -20     # grid of the needs3 exact data


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


# ------------------------------------------------------------- direct conv ----
def direct_inputs(name, N, seed=0, device="cpu", exact=False):
    """``ck.fwd_inputs`` of a direct-conv case; ``exact``: A, w in {-1, 0, 1} and
    an integer bias, so every sum of |terms| is an integer <= 16 C + 3."""
    mode = dc.DIRECT[name][1]
    shape = dc.direct_shape(name, N)
    inp = ck.fwd_inputs(mode, shape, seed=seed, device=device)
    if exact:
        g = _gen(seed + 100, device)
        ri = lambda t, lo, hi: torch.randint(lo, hi + 1, t.shape, generator=g, device=device).to(t.dtype)
        inp["A"], inp["w"], inp["bias"] = ri(inp["A"], -1, 1), ri(inp["w"], -1, 1), ri(inp["bias"], -3, 3)
        from multidisttorch_amd.ops.conv_layout import parity_transpose
        inp["B16"] = (inp["w"].flatten() if mode == dc.CONV else parity_transpose(inp["w"], 2)).contiguous()
    return inp


def direct_out_geom(name, N):
    """(output height = width, columns, output rows per column-sum row, RB)."""
    _, mode, H, C, CO, _, _, R, _ = dc.DIRECT[name]
    oh, ncols, rows = (H // 2, CO, R) if mode == dc.CONV else (H, C, 2 * R)
    return oh, ncols, rows, oh // rows


def direct_colsum_ref(y32, name, N):
    """(ref, bound, cnt) [N RB, ncols]: float64 sums of the y32 pixels of each
    workgroup (see the module docstring) and their bounds."""
    oh, ncols, rows, RB = direct_out_geom(name, N)
    cnt = rows * oh
    v = y32.reshape(N * RB, cnt, ncols).to(F64)
    return v.sum(1), (cnt + SLACK) * EPS * v.abs().sum(1), cnt


# --------------------------------------------------------- weight gradients ----
def dwgrad_shape(name, N):
    _, H, C, CO, _ = dc.DWGRAD[name]
    return (N, H, C, CO, 4, 2, 1)


def dwgrad_inputs(name, N, seed=0, device="cpu", exact=False):
    inp = ck.wgrad_inputs(dwgrad_shape(name, N), seed=seed, device=device)
    if exact:   # {-1, 0, 1}: |terms| sum to <= OH^2 <= 1024 per row, <= 8192 in all
        g = _gen(seed + 100, device)
        for k in ("X", "G"):
            inp[k] = torch.randint(-1, 2, inp[k].shape, generator=g, device=device).to(BF)
    return inp


def check_dwgrad(out, name, N, inp):
    """(worst per-image row ratio, ratio of the float64 row sum): ``ck.check_wgrad``
    with one m-split of OH^2 / 64 tiles per image."""
    sh = dwgrad_shape(name, N)
    return ck.check_wgrad(out, sh, inp, N, (sh[1] // 2) ** 2 // 64)


def thin_inputs(CO, g, x_f32, seed=0, device="cpu"):
    """Single-channel operands: x [N, H, W] (f32 in [0, 1) or bf16 in [-1/2, 1/2)),
    w [CO, 16] f32, bias [CO], G [N, OH, OW, CO] bf16, a bf16 mask of both signs
    with exact zeros [N OH OW, CO], tbias [1], and BCE targets [N, H, W] with
    exact 0 and 1 as well as fractions."""
    N, H, W = g
    gn = _gen(seed, device)
    r = lambda *s: torch.rand(s, generator=gn, device=device)
    rn = lambda *s: torch.randn(s, generator=gn, device=device)
    x = r(N, H, W)
    x = x if x_f32 else (x - 0.5).to(BF)
    M = N * (H // 2) * (W // 2)
    mask = torch.where(r(M, CO) < 0.125, torch.zeros(M, CO, device=device), rn(M, CO)).to(BF)
    tgt = r(N, H, W)
    sel = r(N, H, W)
    tgt = torch.where(sel < 0.2, torch.zeros_like(tgt), torch.where(sel > 0.8, torch.ones_like(tgt), tgt))
    return dict(x=x, w=rn(CO, 16) / 4, bias=rn(CO), G=rn(N, H // 2, W // 2, CO).to(BF), mask=mask,
                tw=rn(CO, 16) / (2 * CO ** 0.5), tbias=rn(1), tgt=tgt.contiguous())


def thin_wgrad_refs(x, G, x_f32):
    """Per partial row (n, 4 output rows): [(ref, bound)] [CO, 16], and the full
    float64 gradient. An f32 x is taken as it is (three exact bf16 terms)."""
    N, H, W = x.shape
    CO = G.shape[-1]
    cols = ck.im2col(x.to(F64).unsqueeze(-1), 4, 2, 1)
    Gm = G.to(F64).reshape(-1, CO)
    step = 4 * (W // 2)
    terms, grow = (3, 1 + 2.0 ** -7) if x_f32 else (1, 1.0)
    slabs = []
    for r0 in range(0, Gm.shape[0], step):
        gg, c = Gm[r0:r0 + step], cols[r0:r0 + step]
        mag = gg.abs().T @ c.abs()
        slabs.append((gg.T @ c, (terms * step + SLACK) * EPS * grow * mag + (2.0 ** -24 * mag if x_f32 else 0)))
    return slabs, Gm.T @ cols


def check_thin_wgrad(out, x, G, x_f32):
    """(worst row ratio, ratio of the float64 row sum against the full gradient)."""
    slabs, full = thin_wgrad_refs(x, G, x_f32)
    got = out[:len(slabs) * full.numel()].view(len(slabs), *full.shape)
    worst = max(ratio(got[i], r, b) for i, (r, b) in enumerate(slabs))
    return worst, ratio(got.to(F64).sum(0), full, sum(b for _, b in slabs))


# ------------------------------------------------------- thin conv / tconv ----
def thin_conv_acc(x, w):
    """(acc, mag) [N OH OW, CO] float64 of the single-channel conv, operands as stored."""
    cols = ck.im2col(x.to(F64).unsqueeze(-1), 4, 2, 1)
    wm = w.to(F64).reshape(w.shape[0], 16)
    return cols @ wm.T, cols.abs() @ wm.abs().T


def thin_epilogue(acc, mag, bias=None, relu=False, mask=None):
    """Bias, ReLU, output mask (kept where mask > 0) on (acc, mag)."""
    ref = acc
    if bias is not None:
        ref, mag = ref + bias.to(F64), mag + bias.to(F64).abs()
    if relu:
        ref = torch.relu(ref)
    if mask is not None:
        ref = torch.where(mask.to(F64).reshape(ref.shape) > 0, ref, torch.zeros_like(ref))
    return ref, mag


def valu_bound(mag, n):
    return (n + SLACK) * U * mag


def conv_mfma_bound(mag):
    return (38 + SLACK) * EPS * mag


def tconv_mfma_bound(mag, CO):
    return (4 * CO + 3 + SLACK) * EPS * mag + 2.0 ** -24 * mag


def thin_conv_bound(mag, CO, g):
    return conv_mfma_bound(mag) if dc.thin_mfma_geom(CO, g) else valu_bound(mag, 17)


def thin_tconv_bound(mag, CO, g):
    return tconv_mfma_bound(mag, CO) if dc.tconv_patch_geom(CO, g) else valu_bound(mag, 4 * CO + 1)


def half_ulp_bf16(v):
    """Half a bf16 unit in the last place of |v| (8 significand bits); TINY at 0."""
    _, e = torch.frexp(v.abs().to(F64))            # |v| = m 2^e, 1/2 <= m < 1: ulp = 2^(e - 8)
    return torch.where(v == 0, torch.full_like(v, TINY, dtype=F64), torch.ldexp(torch.ones_like(v, dtype=F64), e - 9))


def y16_ratio(y16, ref, bound) -> float:
    """y16 is the bf16 rounding of an f32 value within ``bound`` of ``ref``."""
    return ratio(y16.reshape(ref.shape), ref, bound + half_ulp_bf16(ref.abs() + bound))


def thin_colsum_ref(ref, bound):
    """(ref, bound) [blocks, CO] of the per-block column sums of [M, CO] values."""
    M, CO = ref.shape
    nb = -(-M // 256)
    pad = lambda t: F.pad(t, (0, 0, 0, nb * 256 - M)).view(nb, 256, CO)
    r, b = pad(ref), pad(bound)
    return r.sum(1), b.sum(1) + (256 + SLACK) * EPS * r.abs().sum(1)


def thin_tconv_acc(G, w, H, W, bias=None):
    """(logits, mag) [N, H, W] float64 of the one-output-channel transposed conv:
    tap (ky, kx) of input pixel (oy, ox) lands on output (2 oy + ky - 1, 2 ox + kx - 1)."""
    N, OH, OW, CO = G.shape
    g, wm = G.to(F64).reshape(-1, CO), w.to(F64).reshape(CO, 4, 4)
    out = []
    for gg, ww in ((g, wm), (g.abs(), wm.abs())):
        full = torch.zeros((N, 2 * OH + 2, 2 * OW + 2), dtype=F64, device=G.device)
        for ky in range(4):
            for kx in range(4):
                full[:, ky:ky + 2 * OH - 1:2, kx:kx + 2 * OW - 1:2] += (gg @ ww[:, ky, kx]).view(N, OH, OW)
        out.append(full[:, 1:1 + H, 1:1 + W])
    acc, mag = out
    if bias is not None:
        acc, mag = acc + bias.to(F64), mag + bias.to(F64).abs()
    return acc, mag


def tconv_valu_owners(N, H, W, device="cpu"):
    """Flat output pixel indices of every block of the VALU thin_tconv, in block
    order class * gx + x. Class (ca, cb) holds the output pixels of parity
    ((ca + 1) % 2, (cb + 1) % 2), ordered (n, grid row, grid column)."""
    HS, WS = H // 2, W // 2
    own = []
    for cls in range(4):
        oa, ob = (cls // 2 + 1) % 2, (cls % 2 + 1) % 2
        n = torch.arange(N, device=device).view(N, 1, 1)
        iy = (2 * torch.arange(HS, device=device) + oa).view(1, HS, 1)
        ix = (2 * torch.arange(WS, device=device) + ob).view(1, 1, WS)
        px = ((n * H + iy) * W + ix).reshape(-1)
        own += [px[s:s + 256] for s in range(0, px.numel(), 256)]
    return own


def tconv_patch_owners(N, H, W, device="cpu"):
    """Block (n, q) of the halo-patch / MFMA thin_tconv: output rows 8 q .. 8 q + 7 of image n."""
    return [torch.arange(s, s + 8 * W, device=device) for s in range(0, N * H * W, 8 * W)]


def tconv_owners(CO, g, device="cpu"):
    return (tconv_patch_owners if dc.tconv_patch_geom(CO, g) else tconv_valu_owners)(*g, device=device)


def block_partials(v, b_v, owners):
    """(ref, bound) per block: float64 sums of ``v`` over each block's pixels."""
    v, b_v = v.reshape(-1).to(F64), b_v.reshape(-1).to(F64)
    ref = torch.stack([v[o].sum() for o in owners])
    bound = torch.stack([b_v[o].sum() + (o.numel() + SLACK) * U * v[o].abs().sum() for o in owners])
    return ref, bound


def bce_refs(t, b_t, x):
    """The fused BCE at oracle logits ``t`` carrying bound ``b_t``: dict(loss, p,
    g, b_loss, b_p, b_g, b_d16) (see the module docstring)."""
    r = bce_ref(t, x)
    r["b_loss"], r["b_p"], r["b_g"] = r["b_loss"] + b_t, r["b_p"] + b_t / 4, r["b_g"] + b_t / 4
    r["b_d16"] = bf16_bound(r["g"], r["b_g"])
    return r


def check_bce(out, t, b_t, x, owners) -> dict:
    """Ratios of whichever of dlog16, recon, part, gpart ``out`` holds."""
    r = bce_refs(t, b_t, x)
    n, res = t.numel(), {}
    if out.get("dlog16") is not None:
        res["dlog16"] = ratio(out["dlog16"][:n].reshape(t.shape), r["g"], r["b_d16"])
    if out.get("recon") is not None:
        res["recon"] = ratio(out["recon"][:n].reshape(t.shape), r["p"], r["b_p"])
    for key, v, b in (("part", r["loss"], r["b_loss"]), ("gpart", r["g"], r["b_g"])):
        if out.get(key) is not None:
            res[key] = ratio(out[key][:len(owners)], *block_partials(v, b, owners))
    return res


def saturate(tw, G, H, W, tbias, span=150.0):
    """Weights scaled (in f32) so the float64 logits reach beyond [-span, span]."""
    t, _ = thin_tconv_acc(G, tw, H, W, tbias)
    s = 1.1 * span / float(min(t.max(), -t.min()))
    return (tw * s).float().contiguous()


def saturated_recon_ok(recon, t) -> bool:
    """recon is exactly 0 / 1 where the float64 sigmoid rounds to that in f32."""
    p = torch.sigmoid(t.to(F64)).float()
    rc = recon.reshape(t.shape)
    return bool((rc[p == 0] == 0).all()) and bool((rc[p == 1] == 1).all()) and bool((p == 0).any() and (p == 1).any())


# ---------------------------------------------------------- exact-data cases ----
def exact_fits(mag, unit=1.0) -> bool:
    """Every sum of |terms| stays below 2^24 units of the last place."""
    return bool((mag.to(F64) < 2.0 ** 24 * unit).all())


def needs3(shape, seed, device="cpu"):
    """Odd multiples of 2^-20 in [1/4, 1/2) (19 significant bits) whose three
    bf16 terms are all nonzero (``terms_nonzero``). Rounding to nearest leaves a
    residual of up to 10 bits after hi; where it happens to fit lo's 8 bits
    (lo2 = 0), the value is replaced by the first one of the draw that needs lo2."""
    m = torch.randint(2 ** 17, 2 ** 18, shape, generator=_gen(seed, device), device=device)
    v = ((2 * m + 1).to(F64) * UNIT).float()
    hi, lo, lo2 = split3(v)
    good = (lo != 0) & (lo2 != 0)
    return torch.where(good, v, v[good].reshape(-1)[0])


def split3(v):
    """The kernels' bf16 terms of an f32 tensor (hi, lo, lo2) as f32 tensors."""
    hi = v.to(BF).float()
    lo = (v - hi).to(BF).float()
    return hi, lo, (v - hi - lo).to(BF).float()


def terms_nonzero(v) -> bool:
    hi, lo, lo2 = split3(v)
    nz = v != 0
    return bool(((hi != 0) & (lo != 0) & (lo2 != 0))[nz].all()) and bool((hi + lo + lo2 == v).all())


def sparse_sites(N, H, W, per_band, seed, device="cpu"):
    """A {0, 1} f32 image [N, H, W] with ``per_band`` ones in every band of 8
    rows, the first two on the band's first / last row at columns 0 and W - 1
    (the halo row of the neighbouring workgroup and both padding columns)."""
    g = _gen(seed, device)
    s = torch.zeros((N, H, W), device=device)
    for n in range(N):
        for r0 in range(0, H, 8):
            s[n, r0, 0] = s[n, min(H, r0 + 8) - 1, W - 1] = 1
            rows = torch.randint(r0, min(H, r0 + 8), (per_band - 2,), generator=g, device=device)
            cols = torch.randint(0, W, (per_band - 2,), generator=g, device=device)
            s[n, rows, cols] = 1
    return s


def exact_thin_conv(kind, CO, g, seed=0, device="cpu"):
    """Exact thin_conv data, (x f32 [N, H, W], w [CO, 16], bias [CO], unit):
    "ints": x in {0..3}, w in {-2..2}, integer bias (any body);
    "x3": sparse x needing three terms, w in {-1, 0, 1} (MFMA case (a));
    "w3": sparse x in {0, 1}, w = +-needs3 (MFMA case (b)).
    Sparse so that the 256-pixel column sums stay exact as well."""
    N, H, W = g
    gn = _gen(seed, device)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gn, device=device).float()
    if kind == "ints":
        return ri(0, 3, N, H, W), ri(-2, 2, CO, 16), ri(-3, 3, CO), 1.0
    sites = sparse_sites(N, H, W, 3, seed, device)
    if kind == "x3":
        return sites * needs3((N, H, W), seed + 1, device), ri(-1, 1, CO, 16), torch.zeros(CO, device=device), UNIT
    sign = 2 * ri(0, 1, CO, 16) - 1
    return sites, sign * needs3((CO, 16), seed + 1, device), torch.zeros(CO, device=device), UNIT


def exact_thin_tconv(kind, CO, g, seed=0, device="cpu"):
    """Exact thin_tconv data, (G bf16, w [CO, 16], bias [1], unit): "ints" G in
    {-2..2}, w in {-2..2}; "w3": G in {-1, 0, 1} at one site in sixteen, w = +-needs3."""
    N, H, W = g
    gn = _gen(seed, device)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gn, device=device).float()
    if kind == "ints":
        return ri(-2, 2, N, H // 2, W // 2, CO).to(BF), ri(-2, 2, CO, 16), ri(-3, 3, 1), 1.0
    G = ri(-1, 1, N, H // 2, W // 2, CO) * (ri(0, 15, N, H // 2, W // 2, CO) == 0)
    return G.to(BF), (2 * ri(0, 1, CO, 16) - 1) * needs3((CO, 16), seed + 1, device), torch.zeros(1, device=device), UNIT


def exact_thin_wgrad(x_f32, g, seed=0, device="cpu"):
    """Exact thin_wgrad data, (x [N, H, W], G bf16 [N, OH, OW, 32], unit): f32 x
    needs three terms and G is {-1, 0, 1} at one pixel in thirty-two; bf16 x in {-2..2}."""
    N, H, W = g
    gn = _gen(seed, device)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gn, device=device).float()
    if not x_f32:
        return ri(-2, 2, N, H, W).to(BF), ri(-2, 2, N, H // 2, W // 2, 32).to(BF), 1.0
    G = ri(-1, 1, N, H // 2, W // 2, 32) * (ri(0, 31, N, H // 2, W // 2, 32) == 0)
    return needs3((N, H, W), seed + 1, device), G.to(BF), UNIT


def bits_equal(got, ref64) -> bool:
    """The float64 oracle is representable in the result's type and the result
    equals it, every element (a cancelled sum compares equal whatever its zero's sign)."""
    r = ref64.to(got.dtype).reshape(got.shape)
    return bool((r.to(F64) == ref64.reshape(got.shape)).all()) and bool((got == r).all())


__all__ = [n for n in dir() if not n.startswith("_")]
