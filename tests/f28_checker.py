"""Stage-wise checker of the fused 28x28 conv-VAE step (csrc/kernels/
conv28_fused.h, conv28_pair.h, conv28_fused.hip): chained float64 oracles with
derived per-element bounds, the parameter sets, data sets and cases shared by
tests/unit/test_f28_checker.py (CPU: an f32 emulation passes, every mutated one
fails at its own stage) and tests/gpu/test_conv28_stages.py (the kernels, in
all four step forms).

Chaining. The oracle of a stage reads its inputs from the buffers the step
itself stored for the previous stage, bit for bit, and the weights as the
kernel reads them (the bf16 ``w16`` copies; the f32 masters for enc1 and dec2).
A rounding flip or a mask decision upstream therefore never compounds: each
bound below covers ONE phase's arithmetic. All results are error/bound ratios
(``mlp_checker.ratio``): pass means <= 1. NO bound is measured on a kernel.

Notation (tests/igemm_checker.py, tests/direct_checker.py): EPS = 2^-23 bounds
one addition inside an MFMA accumulator (rounding to nearest or truncating),
U = 2^-24 one correctly rounded VALU operation (fmaf, add), SLACK = 9 covers
the bias add, the exchange / addition of K halves (the paired form splits P3,
P7, Q3 and Q5 in two partial sums which both forms add in the same fixed
order) and second-order terms. ``mag`` is the same operation on the absolute
values of the operands. n products added in ANY order carry at most
n (EPS | U) mag (Higham, Accuracy and Stability, section 4.2), so no bound
depends on how a form splits or orders its sums.

A bf16 output is checked as the bf16 rounding (to nearest) of an f32 value
within the stage bound of the oracle: ``direct_checker.y16_ratio``, plus
HALF_SUB = 2^-134, half the spacing of the bf16 subnormals, which that rule's
half-ulp term does not model. ReLU is 1-Lipschitz: the forward needs no special
case at zero. A backward mask is taken from the STORED activation (> 0), so it
is exact: where the stored activation is 0 the bound is 0 and any nonzero
output counts as infinite. A bias partial is the f32 sum of the masked values
BEFORE their bf16 rounding: the element bounds added, plus
(count + SLACK) U sum|v| for its own additions in any order.

Forward (Pn of conv28_fused.h)
  P0  xb = X[idx[cursor * B + n]]: bitwise.
  P1  enc1 on v_mfma_f32_16x16x4_f32, accumulator seeded with the bias, 16 taps
      of f32 x f32 products: the instruction is a k-ordered fmaf chain, one
      rounding per product-and-add: (16 + SLACK) EPS mag. a1 = bf16(relu(.)).
  P2  enc2, bf16 MFMA, K = 16 taps x 32 channels = 512 exact products, bias
      added after: (512 + SLACK) EPS mag. a2 = bf16(relu(.)).
  P3  head, K = 3136 exact bf16 products per output on v_dot2_f32_bf16 into
      four accumulators per K half, then lane and wave sums and the bias. The
      rounding inside a dot2 (two products and the accumulator) is not
      documented as a single one, so each of its additions is taken like an
      MFMA accumulator's: (3136 + SLACK) EPS mag. mulv is f32.
  P4  eps: ``ops.philox.reparam_eps`` keyed with the step the state holds at
      launch, rtol = atol = EPS_TOL = 1e-5. z = fmaf(eps, sd, mu), sd =
      expf(lv / 2): ``conv_small_checker.reparam_ref``'s b_z = 8 U (|mu| +
      |eps sd|); z16 = bf16(z). kld_part[n] = -0.5 sum_c s_c with s_c =
      kl_sum_fma, or -2 fb where the element is floored (-0.5 s_c < fb, fb > 0):
      per element reparam_ref's b_k (0 where floored: fb is exact), plus
      (32 + SLACK) U sum|term| for the wave sum. The floored set is the float64
      one, kl_d < fb, from the stored mulv; the tests keep every element away
      from the floor (``free_bits_cases.check_floor``), so the kernel must
      floor exactly that set.
  P5  dec_fc, one bf16 MFMA of K = 32, bias after: (32 + SLACK) EPS mag.
  P6  dec1 (transposed conv), at most 2 x 2 taps x 64 channels = 256 exact
      products per output: (256 + SLACK) EPS mag.
  P7  dec2 logits, two fmaf chains of f32 weights x bf16 activations (at most
      4 taps x 16 channels each), added, plus the bias: 128 products, 2 adds:
      ``direct_checker.valu_bound(mag, 129)`` = (129 + SLACK) U mag = b_t.
      ``conv_small_checker.bce_ref`` at the oracle's logit gives loss, p, g and
      the bounds of the formulas' own roundings (expf, log1pf, the division).
      b_t enters the loss through |d loss / d t| = |p - x| <= 1, and p and g
      through d p / d t = p (1 - p) <= min(1/4, min(p, 1 - p)), which changes
      by at most e^(b_t) over the interval: b_t min(1/4, min(p, 1 - p) e^b_t).
      (direct_checker's flat b_t / 4 would hide a saturated p: at t = -25,
      p = 1.4e-11.) dlog32 = g, recon = p; bce_part[n] and db4_part[n] are the
      sums of loss and g over the 784 pixels: the pixel bounds added plus
      (784 + SLACK) U sum|v| (``direct_checker.block_partials``).

Backward (Qn)
  Q1  gd1 = [d1 > 0] conv(dlog32, W4f), f32 MFMA as P1 without the seed:
      (16 + SLACK) EPS mag; gd1 = bf16(.); db3_part[n][c] over 196 pixels.
  Q2  gd0 = [d0 > 0] conv(gd1, W3), bf16 MFMA, K = 512: (512 + SLACK) EPS mag.
      dbd_part holds the masked f32 value itself, and gd0 is its bitwise bf16
      twin (``igemm_checker.twin_ok``).
  Q3 + Q4  dz = gd0 . Wd, fmaf chains over 3136 exact products, lane / wave /
      half sums: b_dz = (3136 + SLACK) U mag. d[mu | lv] by
      ``conv_small_checker.reparam_bwd_ref`` with b_dz, the KL weight the
      kernel read (TrainState.kl_next) and weight 0 on the floored set;
      dmulv16 is the bitwise twin of dmulv.
  Q5  ga2 = [a2 > 0] dmulv . Wh with the F32 dmulv (both bodies multiply the
      f32 LDS copy, not dmulv16): 64 fmaf of f32 x bf16 products in two chains
      and their sum: (65 + SLACK) U mag. db2_part is [2][M][64], one row per
      pixel half (pixels 0..23 | 24..48): the two rows are added in float64 and
      compared with the sum over all 49 pixels, (49 + SLACK) U sum|v|.
  Q6  ga1 = [a1 > 0] tconv(ga2, W2), bf16 MFMA, K <= 256: (256 + SLACK) EPS
      mag; db1_part[n][c] over 196 pixels.

Weight-gradient launch + finalize (gradients left in the arena: f28_skip_adam)
  Each layer's (G, X) operand pair as ``_plan28`` wires it, in conv view
  (``WG_SHAPES``); an f32 X (xb, dlog32) is rounded to bf16 by the gather
  (``igemm_checker.as64``). ``igemm_checker.check_wgrad``'s rule: m-split slab
  s within (rows_s + SLACK) EPS mag_s of its float64 value, and the float64
  sum of the slabs within the summed bounds of the full gradient. The
  finalized gradient is the f32 sum of the nsplit slab values in any order:
  (nsplit + SLACK) U sum|slab| of the float64 sum of the STORED slabs.
  Bias gradients: the float64 sum of the stored partial rows (M rows; 2 M for
  enc2; the head's are dmulv), (rows + SLACK) U sum|row|.
  Loss: bce + kl_t kld with both sums over the M stored partials in any order:
  (M + SLACK) U (sum|bce_part| + |kl_t| sum|kld_part|) of their float64 value.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from tests import direct_checker as dc
from tests import igemm_checker as ck
from tests.conv_small_checker import BF16_FILL, EPS_TOL, bce_ref, reparam_bwd_ref, reparam_ref  # noqa: F401
from tests.direct_checker import y16_ratio
from tests.igemm_checker import BF, EPS, F64, SLACK, same_bits, twin_ok  # noqa: F401
from tests.mlp_checker import U, ratio

HALF_SUB = 2.0 ** -134   # half the spacing of the bf16 subnormals
FLAT = 3136              # 7 * 7 * 64

# (G, X) of each layer's weight gradient as _plan28 wires them, and the conv-view descriptor
# (H, C, CO, k, s, p) of igemm_cases (N = M is put in front)
WG_SRCS = {"enc1": ("ga1", "xb"), "enc2": ("ga2", "a1"), "enc_head": ("dmulv16", "a2"),
           "dec_fc": ("gd0", "z16"), "dec1": ("d0", "gd1"), "dec2": ("d1", "dlog32")}
WG_SHAPES = {"enc1": (28, 1, 32, 4, 2, 1), "enc2": (14, 32, 64, 4, 2, 1), "enc_head": (1, FLAT, 64, 1, 1, 0),
             "dec_fc": (1, 32, FLAT, 1, 1, 0), "dec1": (14, 32, 64, 4, 2, 1), "dec2": (28, 1, 32, 4, 2, 1)}
# bias gradient <- its partial buffer (rows per sample)
BIAS_SRCS = {"enc1": ("db1_part", 1), "enc2": ("db2_part", 2), "enc_head": ("dmulv", 1), "dec_fc": ("dbd_part", 1),
             "dec1": ("db3_part", 1), "dec2": ("db4_part", 1)}

# elements per sample of every per-sample buffer of the step, and its dtype
BUFS = {"xb": (784, "f"), "a1": (6272, "b"), "a2": (FLAT, "b"), "mulv": (64, "f"), "eps": (32, "f"), "z16": (32, "b"),
        "d0": (FLAT, "b"), "d1": (6272, "b"), "dlog32": (784, "f"), "bce_part": (1, "f"), "kld_part": (1, "f"),
        "db4_part": (1, "f"), "gd1": (6272, "b"), "db3_part": (32, "f"), "gd0": (FLAT, "b"), "dbd_part": (FLAT, "f"),
        "dmulv": (64, "f"), "dmulv16": (64, "b"), "ga2": (FLAT, "b"), "db2_part": (128, "f"), "ga1": (6272, "b"),
        "db1_part": (32, "f")}
SHAPES = {"a1": (196, 32), "d1": (196, 32), "gd1": (196, 32), "ga1": (196, 32)}
RELU_LAYERS = ("a1", "a2", "d0", "d1")


# ------------------------------------------------------------- data and cases ----
def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def make_data(kind: str, n: int = 512, seed: int = 7) -> torch.Tensor:
    """[n, 784] f32 on the CPU. ``rand``: uniform [0, 1). ``mnist``: blurred
    strokes clamped to [0, 1] inside a 4-pixel border of exact 0.0, with exact
    1.0 pixels. ``bin``: the Bernoulli resampling of ``mnist``, x in {0, 1}."""
    g = gen(seed)
    if kind == "rand":
        return torch.rand(n, 784, generator=g)
    yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
    cy = 8 + 12 * torch.rand(n, 3, 1, 1, generator=g)
    cx = 8 + 12 * torch.rand(n, 3, 1, 1, generator=g)
    blob = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 9.0).sum(1)
    img = torch.clamp(1.6 * blob - 0.1, 0.0, 1.0)
    img[:, :4, :], img[:, -4:, :], img[:, :, :4], img[:, :, -4:] = 0.0, 0.0, 0.0, 0.0
    img = img.reshape(n, 784).contiguous()
    if kind == "mnist":
        return img
    assert kind == "bin", kind
    return (torch.rand(n, 784, generator=g) < img).float()


def make_idx(n: int = 512, seed: int = 8) -> torch.Tensor:
    return torch.randperm(n, generator=gen(seed)).to(torch.int32)


# weight scale and bias size per layer of the ``spread`` set
SPREAD = {"enc1": (2.0, 0.2), "enc2": (2.0, 0.2), "enc_head": (3.0, 0.3), "dec_fc": (2.0, 0.3), "dec1": (3.0, 0.3),
          "dec2": (8.0, 0.5)}


def spread_params(P: dict, seed: int = 11) -> dict:
    """``spread``: the initial weights scaled per layer and every bias replaced
    by a nonzero value of random sign and size in [0.5, 1.5] x the layer's bias
    size, so that the bias adds, the dead-ReLU paths and the saturated BCE
    branch all carry weight (conditions: ``input_conditions``)."""
    g = gen(seed)
    out = {}
    for name, t in P.items():
        ws, bs = SPREAD[name.split(".")[0]]
        t = t.detach().float().cpu()
        if name.endswith(".bias"):
            sign = torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0)
            out[name] = (sign * bs * (0.5 + torch.rand(t.shape, generator=g))).float()
        else:
            out[name] = (t * ws).float()
    return out


def input_conditions(b: dict, W: dict, spread: bool, exact0: bool = False) -> dict:
    """The conditions a case's stored buffers must meet (asserted on the CPU
    emulation and again on the GPU run), name -> bool: finite logits (the
    float64 ones of the stored d1); for ``spread`` also 10 % .. 90 % zeros in
    each ReLU layer, |t| > 20 and |t| < 1 logits, logvar in [-6, 4] and, on
    data with exact zeros (``exact0``: mnist, bin), some t < -20 under x == 0:
    the saturated branch of p."""
    t, _ = logits_ref(b, W)
    out = {"finite": bool(torch.isfinite(t).all() and torch.isfinite(b["dlog32"]).all()
                          and torch.isfinite(b["mulv"]).all())}
    if not spread:
        return out
    for k in RELU_LAYERS:
        z = float((b[k].float() == 0).double().mean())
        out["zeros." + k] = 0.10 <= z <= 0.90
    out["sat"] = bool((t.abs() > 20).any())
    if exact0:
        out["sat0"] = bool(((t < -20) & (b["xb"].reshape(t.shape) == 0)).any())
    out["lin"] = bool((t.abs() < 1).any())
    lv = b["mulv"][:, 32:]
    out["logvar"] = bool((lv >= -6).all() and (lv <= 4).all())
    return out


# (id, B, M, params, data, cursor, step, knobs) -- every case runs on the four step forms
CASES = [
    ("m1-init-rand", 128, 1, "init", "rand", 0, 0, {}),
    ("m2-spread-mnist", 128, 2, "spread", "mnist", 0, 0, {}),
    ("m3-spread-bin", 128, 3, "spread", "bin", 2, 5, {}),
    ("m77-spread-mnist", 128, 77, "spread", "mnist", 1, 3, {}),
    ("m128-spread-rand", 128, 128, "spread", "rand", 0, 0, {}),
    ("m128-init-mnist", 128, 128, "init", "mnist", 3, 0, {}),
    ("m77-kl", 128, 77, "spread", "rand", 1, 4, {"kl_beta": 0.5, "kl_anneal_steps": 16}),
    ("m77-fb", 128, 77, "spread", "mnist", 1, 2, {"free_bits": True}),
    ("b8-m5-spread-bin", 8, 5, "spread", "bin", 1, 1, {}),
    ("b8-m8-spread-mnist", 8, 8, "spread", "mnist", 2, 7, {}),
]
NBATCH = 4   # batches of the index list every case binds (512 rows at B = 128)


# ------------------------------------------------------------------ weights ----
def weights_of(P: dict) -> dict:
    """The kernel's twelve weight tensors from named f32 parameters (arena
    layout [O][kh][kw][I]): bf16 copies, f32 masters for enc1 and dec2."""
    r = lambda t: t.detach().float().cpu().to(BF)
    f = lambda t: t.detach().float().cpu()
    return {"W1f": f(P["enc1.weight"]).reshape(32, 4, 4, 1), "b1": f(P["enc1.bias"]),
            "W2": r(P["enc2.weight"]).reshape(64, 4, 4, 32), "b2": f(P["enc2.bias"]),
            "Wh": r(P["enc_head.weight"]).reshape(64, FLAT), "bh": f(P["enc_head.bias"]),
            "Wd": r(P["dec_fc.weight"]).reshape(FLAT, 32), "bd": f(P["dec_fc.bias"]),
            "W3": r(P["dec1.weight"]).reshape(64, 4, 4, 32), "b3": f(P["dec1.bias"]),
            "W4f": f(P["dec2.weight"]).reshape(32, 4, 4, 1), "b4": f(P["dec2.bias"])}


W_ORDER = ("W1f", "b1", "W2", "b2", "Wh", "bh", "Wd", "bd", "W3", "b3", "W4f", "b4")
W_VIEW = {"W1f": (32, 4, 4, 1), "W2": (64, 4, 4, 32), "Wh": (64, FLAT), "Wd": (FLAT, 32), "W3": (64, 4, 4, 32),
          "W4f": (32, 4, 4, 1)}


def weights_from_list(ts) -> dict:
    """The same dict from the trainer's pointer-table list (``_f28_weights``): the tensors the launch reads."""
    out = {}
    for k, t in zip(W_ORDER, ts):
        t = t.detach().cpu()
        out[k] = t.reshape(W_VIEW[k]) if k in W_VIEW else t
    return out


# ------------------------------------------------------------------ helpers ----
def _d(t):
    return t.to(F64)


def _y16(got, ref, bound) -> float:
    return y16_ratio(got, ref, bound + HALF_SUB)


def _masked(ref, bound, act):
    m = act.reshape(ref.shape).float() > 0
    z = torch.zeros_like(ref)
    return torch.where(m, ref, z), torch.where(m, bound, z)


def _rowsum(ref, bound, M, count):
    """(ref, bound) [M, C] of per-sample sums over ``count`` rows of [M * count, C] values."""
    r, b = ref.reshape(M, count, -1), bound.reshape(M, count, -1)
    return r.sum(1), b.sum(1) + (count + SLACK) * U * r.abs().sum(1)


def _bits_ratio(ok: bool) -> float:
    return 0.0 if ok else math.inf


def kl64(mulv):
    m = mulv.double()
    mu, lv = m[:, :32], m[:, 32:]
    return 0.5 * (mu * mu + torch.exp(lv) - 1 - lv)


def floored_set(mulv, fb: float):
    """The float64 floored set kl_d < fb ([M, 32] bool; empty for fb = 0)."""
    kl = kl64(mulv)
    return kl < fb if fb > 0 else torch.zeros_like(kl, dtype=torch.bool)


def logits_ref(b, W):
    """(t, b_t) [M, 28, 28] float64 of P7's logits from the stored d1."""
    M = b["d1"].shape[0]
    t, mag = dc.thin_tconv_acc(b["d1"].reshape(M, 14, 14, 32), W["W4f"].reshape(32, 4, 4), 28, 28, W["b4"])
    return t, dc.valu_bound(mag, 129)


def bce_refs(t, b_t, x):
    """bce_ref at the oracle's logit with the logit bound carried through the
    formulas' derivatives (module docstring, P7)."""
    r = bce_ref(t, x)
    slope = torch.minimum(torch.full_like(t, 0.25), torch.minimum(r["p"], 1 - r["p"]) * torch.exp(b_t))
    r["b_loss"] = r["b_loss"] + b_t
    r["b_p"] = r["b_p"] + b_t * slope
    r["b_g"] = r["b_g"] + b_t * slope
    return r


# ------------------------------------------------------------------ forward ----
def check_forward(b: dict, W: dict, rows, seed: int, stream: int, step: int, fb: float = 0.0) -> dict:
    """Ratios of P0 .. P7. ``b``: the stored buffers, M rows each, on the CPU;
    ``rows``: X[idx[cursor * B : cursor * B + M]]; ``step``: the state's step at launch."""
    from multidisttorch_amd.ops.philox import reparam_eps

    M = b["xb"].shape[0]
    out = {}
    out["P0.xb"] = _bits_ratio(same_bits(b["xb"].reshape(M, 784), rows.reshape(M, 784).float()))
    # P1
    x = _d(b["xb"]).reshape(M, 28, 28, 1)
    w = _d(W["W1f"])
    ref, mag = ck.conv_ref(x, w, 2, 1) + _d(W["b1"]), ck.conv_ref(x.abs(), w.abs(), 2, 1) + _d(W["b1"]).abs()
    out["P1.a1"] = _y16(b["a1"].reshape(-1, 32), torch.relu(ref), (16 + SLACK) * EPS * mag)
    # P2
    a, w = _d(b["a1"]).reshape(M, 14, 14, 32), _d(W["W2"])
    ref, mag = ck.conv_ref(a, w, 2, 1) + _d(W["b2"]), ck.conv_ref(a.abs(), w.abs(), 2, 1) + _d(W["b2"]).abs()
    out["P2.a2"] = _y16(b["a2"].reshape(-1, 64), torch.relu(ref), (512 + SLACK) * EPS * mag)
    # P3
    a, w = _d(b["a2"]).reshape(M, FLAT), _d(W["Wh"])
    ref, mag = a @ w.T + _d(W["bh"]), a.abs() @ w.abs().T + _d(W["bh"]).abs()
    out["P3.mulv"] = ratio(b["mulv"], ref, (FLAT + SLACK) * EPS * mag)
    # P4
    want = torch.from_numpy(reparam_eps(M, 32, seed, stream, step).astype(np.float64))
    err = (b["eps"].double() - want).abs()
    out["P4.eps"] = float((err / (EPS_TOL + EPS_TOL * want.abs())).max()) if bool(torch.isfinite(err).all()) else math.inf
    z, k, _, b_z, b_k = reparam_ref(b["mulv"], b["eps"])
    out["P4.z16"] = _y16(b["z16"], z, b_z)
    fl = floored_set(b["mulv"], fb)
    term = torch.where(fl, torch.full_like(k, fb), k)
    b_term = torch.where(fl, torch.zeros_like(b_k), b_k)
    out["P4.kld_part"] = ratio(b["kld_part"].reshape(M), term.sum(1),
                               b_term.sum(1) + (32 + SLACK) * U * term.abs().sum(1))
    # P5
    a, w = _d(b["z16"]), _d(W["Wd"])
    ref, mag = a @ w.T + _d(W["bd"]), a.abs() @ w.abs().T + _d(W["bd"]).abs()
    out["P5.d0"] = _y16(b["d0"].reshape(M, FLAT), torch.relu(ref), (32 + SLACK) * EPS * mag)
    # P6
    a, w = _d(b["d0"]).reshape(M, 7, 7, 64), _d(W["W3"])
    ref = ck.tconv_ref(a, w, 2, 1, 14) + _d(W["b3"])
    mag = ck.tconv_ref(a.abs(), w.abs(), 2, 1, 14) + _d(W["b3"]).abs()
    out["P6.d1"] = _y16(b["d1"].reshape(-1, 32), torch.relu(ref), (256 + SLACK) * EPS * mag)
    # P7
    t, b_t = logits_ref(b, W)
    r = bce_refs(t, b_t, _d(b["xb"]).reshape(M, 28, 28))
    out["P7.dlog32"] = ratio(b["dlog32"].reshape(M, 28, 28), r["g"], r["b_g"])
    if b.get("recon") is not None:
        out["P7.recon"] = ratio(b["recon"].reshape(M, 28, 28), r["p"], r["b_p"])
    own = [torch.arange(n * 784, (n + 1) * 784) for n in range(M)]
    out["P7.bce_part"] = ratio(b["bce_part"].reshape(M), *dc.block_partials(r["loss"], r["b_loss"], own))
    out["P7.db4_part"] = ratio(b["db4_part"].reshape(M), *dc.block_partials(r["g"], r["b_g"], own))
    return out


# ----------------------------------------------------------------- backward ----
def check_backward(b: dict, W: dict, klw: float, fb: float = 0.0) -> dict:
    """Ratios of Q1 .. Q6; ``klw`` / ``fb``: the KL weight and the floor as the kernel read them."""
    M = b["xb"].shape[0]
    out = {}
    # Q1
    g, w = _d(b["dlog32"]).reshape(M, 28, 28, 1), _d(W["W4f"])
    ref, mag = ck.conv_ref(g, w, 2, 1), ck.conv_ref(g.abs(), w.abs(), 2, 1)
    ref, bound = _masked(ref, (16 + SLACK) * EPS * mag, b["d1"])
    out["Q1.gd1"] = _y16(b["gd1"].reshape(-1, 32), ref, bound)
    out["Q1.db3_part"] = ratio(b["db3_part"].reshape(M, 32), *_rowsum(ref, bound, M, 196))
    # Q2
    g, w = _d(b["gd1"]).reshape(M, 14, 14, 32), _d(W["W3"])
    ref, mag = ck.conv_ref(g, w, 2, 1), ck.conv_ref(g.abs(), w.abs(), 2, 1)
    ref, bound = _masked(ref, (512 + SLACK) * EPS * mag, b["d0"])
    out["Q2.dbd_part"] = ratio(b["dbd_part"].reshape(-1, 64), ref, bound)
    out["Q2.gd0"] = _bits_ratio(twin_ok(b["gd0"].reshape(-1), b["dbd_part"].reshape(-1)))
    # Q3 + Q4
    g, w = _d(b["gd0"]).reshape(M, FLAT), _d(W["Wd"])
    dz, b_dz = g @ w, (FLAT + SLACK) * U * (g.abs() @ w.abs())
    fl = floored_set(b["mulv"], fb)
    beta = torch.where(fl, torch.zeros_like(dz), torch.full_like(dz, klw))
    out["Q4.dmulv"] = ratio(b["dmulv"], *reparam_bwd_ref(dz, b["mulv"], b["eps"], beta, b_dz))
    out["Q4.dmulv16"] = _bits_ratio(twin_ok(b["dmulv16"].reshape(-1), b["dmulv"].reshape(-1)))
    # Q5
    g, w = _d(b["dmulv"]), _d(W["Wh"])
    ref, bound = _masked(g @ w, (65 + SLACK) * U * (g.abs() @ w.abs()), b["a2"])
    out["Q5.ga2"] = _y16(b["ga2"].reshape(M, FLAT), ref, bound)
    got = b["db2_part"].reshape(2, M, 64).double().sum(0)
    out["Q5.db2_part"] = ratio(got, *_rowsum(ref.reshape(M * 49, 64), bound.reshape(M * 49, 64), M, 49))
    # Q6
    g, w = _d(b["ga2"]).reshape(M, 7, 7, 64), _d(W["W2"])
    ref, mag = ck.tconv_ref(g, w, 2, 1, 14), ck.tconv_ref(g.abs(), w.abs(), 2, 1, 14)
    ref, bound = _masked(ref, (256 + SLACK) * EPS * mag, b["a1"])
    out["Q6.ga1"] = _y16(b["ga1"].reshape(-1, 32), ref, bound)
    out["Q6.db1_part"] = ratio(b["db1_part"].reshape(M, 32), *_rowsum(ref, bound, M, 196))
    return out


# ---------------------------------------------------- weight-gradient launch ----
def wg_inputs(b: dict, name: str) -> dict:
    """The (G, X) pair of layer ``name`` in conv view (NHWC), as check_wgrad takes them."""
    M = b["xb"].shape[0]
    H, C, CO, k, s, p = WG_SHAPES[name]
    OH = (H + 2 * p - k) // s + 1
    gk, xk = WG_SRCS[name]
    return dict(G=b[gk].reshape(M, OH, OH, CO), X=b[xk].reshape(M, H, H, C))


def check_grads(b: dict, grads: dict, slabs: dict, loss, klw: float) -> dict:
    """Ratios of the weight-gradient launch and the finalize. ``grads``: every
    tensor of named_grads(); ``slabs``: layer -> (slab tensor f32, nsplit,
    mt_per_split) of the plan; ``loss``: the step's entry of loss_history()."""
    M = b["xb"].shape[0]
    out = {}
    for name, (H, C, CO, k, s, p) in WG_SHAPES.items():
        slab, ns, mps = slabs[name]
        numel = CO * k * k * C
        worst, total = ck.check_wgrad(slab, (M, H, C, CO, k, s, p), wg_inputs(b, name), ns, mps)
        out[f"WG.{name}.slabs"], out[f"WG.{name}.sum"] = worst, total
        sl = slab[:ns * numel].reshape(ns, numel).double()
        out[f"WG.{name}.weight"] = ratio(grads[name + ".weight"].reshape(numel), sl.sum(0),
                                         (ns + SLACK) * U * sl.abs().sum(0))
        key, per = BIAS_SRCS[name]
        rows = b[key].double().reshape(per * M, -1)
        out[f"WG.{name}.bias"] = ratio(grads[name + ".bias"].reshape(-1), rows.sum(0),
                                       (per * M + SLACK) * U * rows.abs().sum(0))
    bce, kld = b["bce_part"].double().reshape(M), b["kld_part"].double().reshape(M)
    ref = bce.sum() + klw * kld.sum()
    bound = (M + SLACK) * U * (bce.abs().sum() + abs(klw) * kld.abs().sum())
    out["WG.loss"] = ratio(torch.tensor(float(loss), dtype=F64), ref, bound)
    return out


def check_step(b, W, grads, slabs, loss, rows, seed, stream, step, klw, fb=0.0) -> dict:
    out = check_forward(b, W, rows, seed, stream, step, fb)
    out.update(check_backward(b, W, klw, fb))
    out.update(check_grads(b, grads, slabs, loss, klw))
    return out


def stage_of(key: str) -> str:
    return key.split(".")[0]


STAGES = ("P0", "P1", "P2", "P3", "P4", "P5", "P6", "P7", "Q1", "Q2", "Q4", "Q5", "Q6", "WG")


KNOB_STAGES = ("AD", "EM")   # after a shipped step: Adam and the weight average (tests/knob_cases.py)


def first_failure(ratios: dict):
    """The first stage (in step order) with a ratio > 1, or None."""
    for st in STAGES + KNOB_STAGES:
        if any(not r <= 1 for k, r in ratios.items() if stage_of(k) == st):
            return st
    return None
