"""Stage-wise checker of the layer-by-layer conv-VAE step (models/conv_layers.py:
``_forward_hip``, ``_backward_hip``, ``_plan``, the finalize tables, the job
fusion and the deferred transposed-weight copies), generic over
``conv_vae_spec`` (28x28 with any accepted z, 128x128): chained float64 oracles
with derived per-element bounds, the parameter sets, data sets and cases shared
by tests/unit/test_layer_checker.py (CPU: an f32 emulation passes, every
mutated one fails at its own stage) and tests/gpu/test_conv_layer_stages.py
(the kernels, in every step form).

Chaining. The oracle of a stage reads its inputs from the buffers the step
itself stored for the previous stage, bit for bit, and the weights as the
kernel reads them (the bf16 ``w16`` copies; the f32 masters for the two
single-channel edge layers). A rounding flip or a mask decision upstream never
compounds: each bound covers ONE kernel's arithmetic, and every element is
compared. All results are error/bound ratios (``mlp_checker.ratio``): pass
means <= 1. NO bound is measured on a kernel.

Which kernel. For each layer and direction the checker asks the real planner
(``igemm_plan`` / ``wgrad_plan`` on the layer's conv-view descriptor, with the
``allow_split`` / ``fwd`` arguments the step passes) and applies that kernel's
existing rule. Notation (tests/igemm_checker.py, tests/direct_checker.py):
EPS = 2^-23 bounds one addition inside an MFMA accumulator, U = 2^-24 one
correctly rounded VALU operation, SLACK = 9; ``mag`` is the same operation on
the absolute values of the operands; n products added in ANY order carry at
most n (EPS | U) mag (Higham, Accuracy and Stability, section 4.2).

  cfg 0..7 (igemm_fwd_k)      ``igemm_checker.fwd_bound(mag, K, ksplit)`` =
                              (K + ksplit + SLACK) EPS mag; K is the planner's.
  cfg 100..105 (dconv_body)   operands are bf16, products exact:
                              direct_checker's docstring applies fwd_bound
                              unchanged with K = 16 C (conv) or 4 CO (one
                              parity class), the planner's K again.
  thin_conv (first layer, and the last layer's backward-data)
                              ``direct_checker.thin_conv_bound``: (38 + SLACK)
                              EPS mag on the MFMA body (CO = 32, W = 128),
                              (17 + SLACK) U mag on the VALU body; f32 weights
                              and an f32 input are read as stored.
  thin_tconv (last layer)     ``direct_checker.thin_tconv_bound``; the fused
                              BCE by ``direct_checker.check_bce`` with
                              ``tconv_owners``: dlog16, recon, the bce_part
                              blocks and gpart.
  raw split-K slab s          (K_s + SLACK) EPS mag_s over its own k-tiles
                              (``igemm_checker.slab_refs``' rule; a Linear
                              layer's k index is its input feature).
  combine of ks slabs         ``conv_small_checker.slab_sum_ref`` on the STORED
                              slabs: (ks + 4) U (sum|slab| + |bias|).
  reparameterisation          ``reparam_ref`` (z: 8 U (|mu| + |eps sd|), bf16
                              store), eps against ``ops.philox.reparam_eps`` at
                              EPS_TOL keyed with the state's step at launch, the
                              KLD partial of each block of ``block_owners`` by
                              ``block_sum_ref``; a floored element (float64
                              kl_d < fb, from the stored mulv) adds exactly fb.
  reparameterisation backward ``reparam_bwd_ref`` from the STORED dz, with the
                              KL weight the state held and weight 0 on the
                              floored set; dmulv16 is the bitwise twin of dmulv.
                              With the total-correlation penalty (``tc``) the
                              reference gains tc_t g64 (``knob_cases.tc_rule``).

A bf16 output is checked as the bf16 rounding of an f32 value within the stage
bound of the oracle (``direct_checker.y16_ratio``) plus HALF_SUB = 2^-134, half
the spacing of the bf16 subnormals. ReLU is 1-Lipschitz. A backward mask is
taken from the STORED activation (> 0), so it is exact: where the stored
activation is 0 the bound is 0 and any nonzero output counts as infinite.

Bias partial rows (``colsum`` of the plan): the f32 sum of the masked values
BEFORE their bf16 rounding, so the element bounds added plus
(count + SLACK) U sum|v| for the row's own additions in any order; count is
the largest number of values any row of that buffer sums. The rows are
  cfg 0..7    (class, m-tile): BM consecutive GEMM rows; parity-class rows are
              mapped to pixels by ``igemm_checker.parity_rows``;
  cfg 100..   ``colsum_rows`` equal blocks of consecutive NHWC pixels
              (direct_checker: workgroup (n, rb));
  thin_conv   blocks of 256 consecutive pixels.
The two Linear biases come from the ``colsum`` kernel: row y is the f32 sum of
rows 8 y .. 8 y + 7 of the bf16 gradient as stored: (8 + SLACK) U sum|v|.

Weight gradients. Each layer's (G, X) pair as ``_backward_hip`` wires it, in
conv view: conv / Linear layers G = the gradient of the layer's output, X =
its input; transposed-conv layers the other way round (G = the layer's input
activation, X = the gradient of its output). cfg 0..5: ``igemm_checker.
check_wgrad`` (m-split slab s within (rows_s + SLACK) EPS mag_s, an f32 X is
rounded to bf16 by the gather); cfg 100 / 101: one slab per image
(``direct_checker.check_dwgrad``'s rule); cfg 110: ``check_thin_wgrad`` (one
slab per image and four output rows, an f32 X as stored). The float64 slab sum
is checked against the full gradient under the summed bounds, the arena
gradient is within (nsplit + SLACK) U sum|slab| of the float64 sum of the
STORED slabs, each bias gradient within (rows + SLACK) U sum|row| of the
float64 sum of its stored partial rows, and the loss within
(nb + nk + SLACK) U (sum|bce_part| + |kl_t| sum|kld_part|) of bce + kl_t kld.

What a form cannot show. enc2's own split-K slabs at 28x28 are combined inside
its launch and the head's slabs overwrite them in the same workspace: enc2 is
checked through its output under the split-K bound. The head's forward slabs
survive only where nothing runs after the forward (the copy the manual forms
take, and the eval pass); elsewhere ``mulv`` is checked against the full
product under (K + ksplit + SLACK) EPS mag. The last layer of both image sizes
runs on thin_tconv with the fused BCE, so ``bce_logits`` is reached by no step
(tests/gpu/test_conv_small_kernels.py covers it); ``logits`` is checked where
``decode()`` stores it. The ``ws_a`` / APro fold of ``_forward_hip`` is
unreachable at the default planner switches (enc3 at 128x128 runs the direct
kernel, 28x28 has two encoder layers), and the switches are read once per
process into statics: neither the fold nor any non-default switch is covered.

Adam. ``conv_small_checker.adam_ref`` from the arena gradient the finalize
kernel itself writes without Adam from the same stored slabs (the fused form
consumes that gradient in registers; ``test_grad_finalize_fused_adam`` feeds
its oracle the same way, so no gradient bound needs to be carried): params,
exp_avg and exp_avg_sq within its bounds, w16 the bitwise bf16 twin of params.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from multidisttorch_amd.models.conv_spec import _w_shape, conv_vae_spec
from tests import direct_checker as dc
from tests import igemm_checker as ck
from tests.conv_small_checker import (BF16_FILL, EPS_TOL, adam_consts, adam_ref, block_owners, block_sum_ref,  # noqa: F401
                                      reparam_bwd_ref, reparam_ref, slab_sum_ref)
from tests.direct_checker import y16_ratio
from tests.f28_checker import gen, make_idx  # noqa: F401
from tests.igemm_checker import BF, EPS, F64, SLACK, same_bits, twin_ok
from tests.mlp_checker import U, ratio

HALF_SUB = 2.0 ** -134   # half the spacing of the bf16 subnormals
ROWS_PER = 8             # rows per partial of the colsum kernel (``_plan``)
NBATCH = 4               # batches of the index list every case binds


# ------------------------------------------------------------------ geometry ----
def desc(l, M):
    """The 11-int conv-view descriptor of a layer (``ConvVaeTrainer._desc``)."""
    if l.kind == "convT":
        return [M, l.out_hw, l.out_hw, l.cout, l.in_hw, l.in_hw, l.cin, l.k, l.k, l.s, l.p]
    return [M, l.in_hw, l.in_hw, l.cin, l.out_hw, l.out_hw, l.cout, l.k, l.k, l.s, l.p]


def shape_of(l, M):
    """(N, H, C, CO, k, s, p) of tests/igemm_cases.py."""
    d = desc(l, M)
    return (M, d[1], d[3], d[6], d[7], d[9], d[10])


def thin_edges(spec):
    """(first, last): the single-channel edge layers run on conv_thin.hip (``_alloc_hip``'s conditions)."""
    f, l = spec[0], spec[-1]
    first = f.kind == "conv" and f.cin == 1 and f.cout in (16, 32, 64) and f.k <= 4
    last = l.kind == "convT" and l.cout == 1 and l.cin in (16, 32, 64) and l.k % l.s == 0 and l.out_hw % l.s == 0
    return first, last


def plans(spec, M):
    """name -> dict(F, D, W) of the planner's answers for batch M as the step asks them; ``"thin"`` for the
    direct single-channel kernels, D None for the first layer."""
    from multidisttorch_amd.ops.conv_plans import igemm_plan, wgrad_plan

    tf, tl = thin_edges(spec)
    out = {}
    for i, l in enumerate(spec):
        d = desc(l, M)
        last = i == len(spec) - 1
        if (i == 0 and tf) or (last and tl):
            F = "thin"
        elif l.kind == "convT":
            F = igemm_plan(1, d, False, fwd=True)
        else:
            F = igemm_plan(0, d, True, fwd=True)
        if i == 0:
            D = None
        elif last and tl:
            D = "thin"
        else:
            D = igemm_plan(0 if l.kind == "convT" else 1, d, l.name == "dec_fc")
        out[l.name] = dict(F=F, D=D, W=wgrad_plan(d))
    return out


def n_bce(spec, M):
    from multidisttorch_amd.ops import native

    return native.require().thin_blocks(True, desc(spec[-1], M))


def bias_rows(spec, M, pl):
    """name -> partial rows the finalize sums for that layer's bias (``_plan``)."""
    from multidisttorch_amd.ops import native

    rows = {}
    for i, l in enumerate(spec):
        if i == 0:
            continue
        prev = spec[i - 1]
        if l.name == "dec_fc" or prev.name == "dec_fc":
            continue
        if pl[l.name]["D"] == "thin":
            rows[prev.name] = native.require().thin_blocks(False, desc(l, M))
        else:
            q = pl[l.name]["D"]
            rows[prev.name] = q.colsum_rows * (q.ncols // prev.cout)
    rows["enc_head"] = rows["dec_fc"] = -(-M // ROWS_PER)
    rows[spec[-1].name] = n_bce(spec, M)
    return rows


def finalize_rp(ns):
    """Partial rows per unit column of the finalize kernel (``_finalize_units``)."""
    rp = 1
    if ns > 1:
        while rp < 256 and rp * 16 < ns:
            rp *= 2
    return rp


def plan_tuples(image, z, M):
    """Every (image, layer, direction, cfg, ksplit > 1, nsplit > 1, finalize rp > 1) of one batch size; direction
    "B" is the bias segment of the finalize (nsplit = its partial rows)."""
    spec = conv_vae_spec(image, 1, z)
    pl = plans(spec, M)
    out = set()
    for l in spec:
        p = pl[l.name]
        for k in ("F", "D"):
            q = p[k]
            if q is not None:
                out.add((image, l.name, k, "thin", False, False, False) if q == "thin" else
                        (image, l.name, k, q.cfg, q.ksplit > 1, False, False))
        w = p["W"]
        out.add((image, l.name, "W", w.cfg, False, w.nsplit > 1, finalize_rp(w.nsplit) > 1))
    for name, r in bias_rows(spec, M, pl).items():
        out.add((image, name, "B", None, False, r > 1, finalize_rp(r) > 1))
    return out


# --------------------------------------------------------------------- cases ----
# (id, image, z, B, M, params, data, cursor, step, knobs). ``small``: the CPU emulation runs them too.
CASES = [
    ("128-m1-init-rand", 128, 64, 8, 1, "init", "rand", 0, 0, {}),
    ("128-m3-spread-mnist", 128, 64, 8, 3, "spread", "mnist", 1, 2, {}),
    ("128-m8-spread-bin", 128, 64, 8, 8, "spread", "bin", 0, 0, {}),
    ("28-m1-init-rand", 28, 32, 16, 1, "init", "rand", 0, 0, {}),
    ("28-m5-spread-mnist", 28, 32, 16, 5, "spread", "mnist", 2, 5, {}),
    ("28-m16-spread-bin", 28, 32, 16, 16, "spread", "bin", 0, 0, {}),
    ("28-z8-m5", 28, 8, 16, 5, "spread", "rand", 0, 0, {}),
    ("28-z24-m5", 28, 24, 16, 5, "spread", "mnist", 1, 1, {}),
    ("28-z128-m5", 28, 128, 16, 5, "spread", "rand", 0, 0, {}),
    ("28-b128-m77", 28, 32, 128, 77, "spread", "mnist", 1, 3, {}),
    ("28-b128-m128", 28, 32, 128, 128, "init", "rand", 0, 0, {}),
    ("28-m5-kl", 28, 32, 16, 5, "spread", "rand", 1, 4, {"kl_beta": 0.5, "kl_anneal_steps": 16}),
    ("28-m16-fb", 28, 32, 16, 16, "spread", "mnist", 1, 2, {"free_bits": True}),
]
SMALL = ("128-m1-init-rand", "128-m3-spread-mnist", "28-m1-init-rand", "28-m5-spread-mnist", "28-z8-m5", "28-z24-m5",
         "28-z128-m5", "28-m5-kl", "28-m16-fb")
# the shipped 128x128 batch: only the stages whose tuple no case above has
BIG = ("128-b64-m64", 128, 64, 64, 64, "init", "rand", 0, 0, {})
# ... which are: enc4's backward-data on cfg 5, and the finalize forms with more than 16 partial rows (the
# per-image slabs of enc2 and dec3) or more than one (the colsum kernel's rows of the two Linear biases)
BIG_ONLY = dict(backward=("enc4",), grads=("enc2", "dec3", "enc_head", "dec_fc"))
# (image, z, B) of the shipped batches the case table must cover
SHIPPED = [(128, 64, 64), (28, 32, 128), (28, 8, 128), (28, 24, 128), (28, 128, 128)]


def case_tuples(cases=None):
    out = set()
    for c in (CASES if cases is None else cases):
        out |= plan_tuples(c[1], c[2], c[4])
    return out


def make_data(kind: str, image: int, n: int = 512, seed: int = 7) -> torch.Tensor:
    """[n, image^2] f32 on the CPU (``f28_checker.make_data`` at any size). ``rand``: uniform [0, 1).
    ``mnist``: blurred strokes clamped to [0, 1] inside a border of exact 0.0, with exact 1.0 pixels.
    ``bin``: the Bernoulli resampling of ``mnist``."""
    g = gen(seed)
    D = image * image
    if kind == "rand":
        return torch.rand(n, D, generator=g)
    sc = image / 28.0
    yy, xx = torch.meshgrid(torch.arange(float(image)), torch.arange(float(image)), indexing="ij")
    cy = (8 + 12 * torch.rand(n, 3, 1, 1, generator=g)) * sc
    cx = (8 + 12 * torch.rand(n, 3, 1, 1, generator=g)) * sc
    blob = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (9.0 * sc * sc)).sum(1)
    img = torch.clamp(1.6 * blob - 0.1, 0.0, 1.0)
    e = int(round(4 * sc))
    img[:, :e, :], img[:, -e:, :], img[:, :, :e], img[:, :, -e:] = 0.0, 0.0, 0.0, 0.0
    img = img.reshape(n, D).contiguous()
    if kind == "mnist":
        return img
    assert kind == "bin", kind
    return (torch.rand(n, D, generator=g) < img).float()


def data_rows(case):
    """Rows of the data set a case binds: NBATCH batches."""
    return NBATCH * case[3]


def spread_params(P: dict, spec, seed: int = 11) -> dict:
    """``f28_checker.spread_params`` for any spec: the initial weights scaled per layer role and every bias
    replaced by a nonzero value of random sign and size in [0.5, 1.5] x the role's bias size, so that the bias
    adds, the dead-ReLU paths and both BCE branches carry weight (``input_conditions``)."""
    role = {}
    for i, l in enumerate(spec):
        if i == len(spec) - 1:
            role[l.name] = (6.0, 0.5)
        elif l.name == "enc_head":
            role[l.name] = (3.0, 0.3)
        elif l.name == "dec_fc":
            role[l.name] = (2.0, 0.3)
        elif l.kind == "convT":
            role[l.name] = (2.0, 0.2)
        else:
            role[l.name] = (2.0, 0.2)
    g = gen(seed)
    out = {}
    for name, t in P.items():
        ws, bs = role[name.split(".")[0]]
        t = t.detach().float().cpu()
        if name.endswith(".bias"):
            sign = torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0)
            out[name] = (sign * bs * (0.5 + torch.rand(t.shape, generator=g))).float()
        else:
            out[name] = (t * ws).float()
    return out


def weights_of(P: dict, spec) -> dict:
    """name -> dict(w, b) as the kernels read them from named f32 parameters: bf16 copies, f32 masters on the
    single-channel edge layers; w in conv view [CO, k, k, C]."""
    tf, tl = thin_edges(spec)
    out = {}
    for i, l in enumerate(spec):
        w = P[l.name + ".weight"].detach().float().reshape(_w_shape(l))
        thin = (i == 0 and tf) or (i == len(spec) - 1 and tl)
        out[l.name] = dict(w=w if thin else w.to(BF), b=P[l.name + ".bias"].detach().float())
    return out


# ------------------------------------------------------------------- helpers ----
def _d(t):
    return t.to(F64)


def _y16(got, ref, bound) -> float:
    return y16_ratio(got, ref, bound + HALF_SUB)


def _bits_ratio(ok: bool) -> float:
    return 0.0 if ok else math.inf


def _masked(ref, bound, act):
    m = act.reshape(ref.shape).float() > 0
    z = torch.zeros_like(ref)
    return torch.where(m, ref, z), torch.where(m, bound, z)


def kl64(mulv):
    m = mulv.double()
    Z = m.shape[1] // 2
    mu, lv = m[:, :Z], m[:, Z:]
    return 0.5 * (mu * mu + torch.exp(lv) - 1 - lv)


def floored_set(mulv, fb: float):
    kl = kl64(mulv)
    return kl < fb if fb > 0 else torch.zeros_like(kl, dtype=torch.bool)


def colsum_owner(q, sh, mode, device="cpu"):
    """(owner [rows of the GEMM output in NHWC order] -> partial row, number of partial rows) of the
    bias column sums a backward-data call writes; ``q``: its plan, "thin", or an int (blocks of the
    thin kernel); ``sh``: the layer's conv-view shape; mode 0 conv (output OH^2 pixels), 1 parity (H^2)."""
    N, H, C, CO, k, s, p = sh
    OH = (H + 2 * p - k) // s + 1
    npx = N * (OH * OH if mode == 0 else H * H)
    ar = torch.arange(npx, device=device)
    if isinstance(q, int):
        return ar // 256, q
    if q.cfg >= 100:
        assert npx % q.colsum_rows == 0
        return ar // (npx // q.colsum_rows), q.colsum_rows
    assert q.colsum_rows == q.classes * q.mtiles
    if mode == 0 or q.classes == 1:
        return ar // q.bm, q.colsum_rows
    own = torch.empty(npx, dtype=torch.long, device=device)
    for c in range(q.classes):
        rows = ck.parity_rows(sh, c, device)
        own[rows] = c * q.mtiles + torch.arange(rows.numel(), device=device) // q.bm
    return own, q.colsum_rows


def owner_sums(v, own, rows):
    """float64 [rows, C] sums of the [n, C] values of each owner."""
    out = torch.zeros((rows, v.shape[1]), dtype=v.dtype, device=v.device)
    return out.index_add_(0, own, v)


def _partials(ref, bound, own, rows):
    cnt = int(torch.bincount(own, minlength=rows).max())
    return owner_sums(ref, own, rows), owner_sums(bound, own, rows) + (cnt + SLACK) * U * owner_sums(ref.abs(), own, rows)


def wg_rows_per_slab(w, sh):
    """GEMM rows (n, oy, ox) each partial slab of a weight-gradient call sums."""
    N, H, C, CO, k, s, p = sh
    OH = (H + 2 * p - k) // s + 1
    if w.cfg == 110:
        return 4 * OH
    if w.cfg >= 100:
        return OH * OH
    return 64 * w.mt_per_split


def wg_pair(spec, i, b):
    """(G, X) of layer i's weight gradient in conv view (NHWC), as ``_backward_hip`` wires them."""
    l = spec[i]
    M = b["xb"].shape[0]
    N, H, C, CO, k, s, p = shape_of(l, M)
    OH = (H + 2 * p - k) // s + 1
    if i == 0:
        a_in = b["xb"]
    elif l.name == "dec_fc":
        a_in = b["z16"]
    else:
        a_in = b["acts"][spec[i - 1].name]
    if i == len(spec) - 1:
        g = b["dlog16"]
    elif l.name == "enc_head":
        g = b["dmulv16"]
    else:
        g = b["gacts"][l.name]
    if l.kind == "convT":
        return a_in.reshape(M, OH, OH, CO), g.reshape(M, H, H, C)
    return g.reshape(M, OH, OH, CO), a_in.reshape(M, H, H, C)


def _lin_slabs(a, w, q):
    """[(ref_s, bound_s)] of a split-K Linear GEMM a [M, K] x w [N, K]^T over its k-tiles."""
    kps = -(-q.ktiles // q.ksplit)
    out = []
    for kt0 in range(0, q.ktiles, kps):
        lo, hi = 64 * kt0, min(q.k, 64 * (kt0 + kps))
        aa, ww = a[:, lo:hi], w[:, lo:hi]
        out.append((aa @ ww.T, (hi - lo + SLACK) * EPS * (aa.abs() @ ww.abs().T)))
    assert len(out) == q.ksplit, (len(out), q.ksplit)
    return out


# ------------------------------------------------------------------- forward ----
def _layer_ref(spec, i, b, W, M):
    """(ref, mag) float64 [rows, cols] of layer i's pre-activation from its stored input."""
    l = spec[i]
    sh = shape_of(l, M)
    N, H, C, CO, k, s, p = sh
    w, bias = W[l.name]["w"], _d(W[l.name]["b"])
    if i == 0:
        x = b["xb"]
        x = x if thin_edges(spec)[0] else x.to(BF)
    elif l.name == "dec_fc":
        x = b["z16"]
    else:
        x = b["acts"][spec[i - 1].name]
    if l.kind == "convT":
        OH = (H + 2 * p - k) // s + 1
        a = _d(x).reshape(M, OH, OH, CO)
        ref, mag = ck.tconv_ref(a, _d(w), s, p, H), ck.tconv_ref(a.abs(), _d(w).abs(), s, p, H)
    else:
        a = _d(x).reshape(M, H, H, C)
        ref, mag = ck.conv_ref(a, _d(w), s, p), ck.conv_ref(a.abs(), _d(w).abs(), s, p)
    return ref + bias, mag + bias.abs()


def _fwd_bound(q, mag, l, M):
    if q == "thin":
        N, H, C, CO, k, s, p = shape_of(l, M)
        return dc.thin_conv_bound(mag, CO, (M, H, H))
    return ck.fwd_bound(mag, q.k, q.ksplit)


def check_forward(spec, b, W, pl, rows, seed, stream, step, fb=0.0, layers=None, want=("enc", "rep", "dec")):
    """Ratios of the forward stages. ``b``: the stored buffers (M rows each); ``rows``: X[idx[cursor B ..]] or
    None; ``step``: the state's step at launch. ``want``: which parts the buffers hold."""
    M = b["xb"].shape[0] if "xb" in b else b["z16"].shape[0]
    dev = b["z16"].device
    Z = b["z16"].shape[1]
    out = {}
    if rows is not None:
        out["F.gather.xb"] = _bits_ratio(same_bits(b["xb"].reshape(M, -1), rows.reshape(M, -1).float().to(dev)))
    tl = thin_edges(spec)[1]
    for i, l in enumerate(spec):
        enc = l.name.startswith("enc")
        if (enc and "enc" not in want) or (not enc and "dec" not in want):
            continue
        q = pl[l.name]["F"]
        last = i == len(spec) - 1
        if l.name == "enc_head":
            a, w = _d(b["acts"][spec[i - 1].name]).reshape(M, -1), _d(W[l.name]["w"]).reshape(2 * Z, -1)
            bias = _d(W[l.name]["b"])
            if q.ksplit > 1 and b.get("ws_fwd") is not None:
                refs = _lin_slabs(a, w, q)
                got = b["ws_fwd"][:q.ksplit * M * 2 * Z].view(q.ksplit, M, 2 * Z)
                out["F.enc_head.slabs"] = max(ratio(got[j], r, bd) for j, (r, bd) in enumerate(refs))
                out["F.enc_head.slab_sum"] = ratio(got.double().sum(0), a @ w.T, sum(bd for _, bd in refs))
                out["F.enc_head.mulv"] = ratio(b["mulv"], *slab_sum_ref(got, bias))
            else:
                ref, mag = a @ w.T + bias, a.abs() @ w.abs().T + bias.abs()
                out["F.enc_head.mulv"] = ratio(b["mulv"], ref, ck.fwd_bound(mag, q.k, q.ksplit))
            if "rep" in want:
                out.update(check_reparam(b, q, seed, stream, step, fb))
            continue
        ref, mag = _layer_ref(spec, i, b, W, M)
        if last and tl:
            N, H, C, CO, k, s, p = shape_of(l, M)
            t, tm = ref.reshape(M, H, H), mag.reshape(M, H, H)
            b_t = dc.thin_tconv_bound(tm, CO, (M, H, H))
            if b.get("logits") is not None:
                out[f"F.{l.name}.logits"] = ratio(b["logits"].reshape(M, H, H), t, b_t)
            if b.get("bce_part") is not None:
                o = dict(dlog16=b.get("dlog16"), recon=b.get("recon"), part=b["bce_part"], gpart=b.get("gpart"))
                o = {k2: (v.reshape(-1) if v is not None else None) for k2, v in o.items()}
                owners = dc.tconv_owners(CO, (M, H, H), device=dev)
                assert len(owners) == b["bce_part"].numel(), (len(owners), b["bce_part"].numel())
                for k2, r in dc.check_bce(o, t, b_t, _d(b["xb"]).reshape(M, H, H), owners).items():
                    out[f"F.{l.name}.{'bce_part' if k2 == 'part' else k2}"] = r
            continue
        assert l.relu and not last
        out[f"F.{l.name}.act"] = _y16(b["acts"][l.name].reshape(ref.shape), torch.relu(ref), _fwd_bound(q, mag, l, M))
    return out


def check_reparam(b, q, seed, stream, step, fb=0.0):
    from multidisttorch_amd.ops.philox import reparam_eps

    M, Z = b["z16"].shape
    dev = b["z16"].device
    out = {}
    want = torch.from_numpy(reparam_eps(M, Z, seed, stream, step).astype(np.float64)).to(dev)
    err = (b["eps"].double() - want).abs()
    out["F.reparam.eps"] = float((err / (EPS_TOL + EPS_TOL * want.abs())).max()) if bool(
        torch.isfinite(err).all()) else math.inf
    z, k, _, b_z, b_k = reparam_ref(b["mulv"], b["eps"])
    out["F.reparam.z16"] = _y16(b["z16"], z, b_z)
    fl = floored_set(b["mulv"], fb)
    term = torch.where(fl, torch.full_like(k, fb), k)
    b_term = torch.where(fl, torch.zeros_like(b_k), b_k)
    owners = block_owners(M, Z, q.ksplit if q.ksplit > 1 else None)
    assert len(owners) == b["kld_part"].numel(), (len(owners), b["kld_part"].numel())
    out["F.reparam.kld_part"] = ratio(b["kld_part"], *block_sum_ref(term, b_term, [o.to(dev) for o in owners]))
    return out


# ------------------------------------------------------------------ backward ----
def dmulv_ref(b, klw, fb=0.0, tc=None):
    """(ref, bound) of d[mu|lv] from the STORED dz, mulv and eps: ``reparam_bwd_ref`` with the KL weight the
    state held and weight 0 on the floored set, then the penalty's share by ``knob_cases.tc_rule``."""
    from tests.knob_cases import tc_rule

    fl = floored_set(b["mulv"], fb)
    beta = torch.where(fl, torch.zeros_like(fl, dtype=F64), torch.full(fl.shape, klw, dtype=F64, device=fl.device))
    return tc_rule(*reparam_bwd_ref(b["dz"], b["mulv"], b["eps"], beta), tc)


def check_backward(spec, b, W, pl, klw, fb=0.0, only=None, tc=None):
    """Ratios of the backward stages B.<layer>: layer's backward-data (the gradient of the previous layer's
    output) and the bias partial rows it emits. ``only``: layer names to check (None: all). ``tc``: (tc_t, g64,
    bg) of ``knob_cases.tc_of`` when the step folds the total-correlation penalty into d[mu|lv] (``tc_fold_k``
    adds in place and rewrites dmulv16): the reference gains ``tc_t g64`` within ``tc_t bg + 2 U max(|before|,
    |after|)``; dmulv16 stays the bitwise twin, and the stages fed from the stored dmulv16 (the head's bias
    partial rows, B.enc_head, WG.enc_head) then show that their kernels consumed the folded value."""
    M, Z = b["z16"].shape
    dev = b["z16"].device
    out = {}
    n = len(spec)
    for i in range(n - 1, 0, -1):
        l, prev = spec[i], spec[i - 1]
        if only is not None and l.name not in only:
            continue
        q = pl[l.name]["D"]
        sh = shape_of(l, M)
        N, H, C, CO, k, s, p = sh
        w = W[l.name]["w"]
        g = b["dlog16"] if i == n - 1 else (b["dmulv16"] if l.name == "enc_head" else b["gacts"][l.name])
        tag = f"B.{l.name}."
        if l.name == "dec_fc":
            gm, wm = _d(g).reshape(M, -1), _d(w).reshape(-1, Z)          # [M, flat], [flat, Z]
            if q.ksplit > 1:
                refs = _lin_slabs(gm, wm.T.contiguous(), q)
                got = b["ws_bwd"][:q.ksplit * M * Z].view(q.ksplit, M, Z)
                out[tag + "slabs"] = max(ratio(got[j], r, bd) for j, (r, bd) in enumerate(refs))
                out[tag + "slab_sum"] = ratio(got.double().sum(0), gm @ wm, sum(bd for _, bd in refs))
                out[tag + "dz"] = ratio(b["dz"], *slab_sum_ref(got))
            else:
                out[tag + "dz"] = ratio(b["dz"], gm @ wm, ck.fwd_bound(gm.abs() @ wm.abs(), q.k))
            out[tag + "dmulv"] = ratio(b["dmulv"], *dmulv_ref(b, klw, fb, tc))
            out[tag + "dmulv16"] = _bits_ratio(twin_ok(b["dmulv16"].reshape(-1), b["dmulv"].reshape(-1)))
            # the head's bias partials: the colsum kernel over the bf16 gradient
            out[tag + "colsum"] = _colsum16(b["dmulv16"], b["colsum"]["enc_head"])
            continue
        if q == "thin":     # the last layer's backward-data: single-channel conv of dlog16 with the f32 weights
            ref, mag = dc.thin_conv_acc(g.reshape(M, H, H), w.reshape(CO, 16))
            bound = dc.thin_conv_bound(mag, CO, (M, H, H))
            mode = 0
            qq = b["colsum"][prev.name].numel() // CO
        elif l.kind == "convT":
            gg = _d(g).reshape(M, H, H, C)
            ref, mag = ck.conv_ref(gg, _d(w), s, p), ck.conv_ref(gg.abs(), _d(w).abs(), s, p)
            bound, mode, qq = ck.fwd_bound(mag, q.k), 0, q
        else:
            OH = (H + 2 * p - k) // s + 1
            gg = _d(g).reshape(M, OH, OH, CO)
            ref, mag = ck.tconv_ref(gg, _d(w), s, p, H), ck.tconv_ref(gg.abs(), _d(w).abs(), s, p, H)
            bound, mode, qq = ck.fwd_bound(mag, q.k), 1, q
        if prev.relu:
            ref, bound = _masked(ref, bound, b["acts"][prev.name])
        out[tag + "gin"] = _y16(b["gacts"][prev.name].reshape(ref.shape), ref, bound)
        if prev.name == "dec_fc":
            out[tag + "colsum"] = _colsum16(b["gacts"][prev.name].reshape(M, -1), b["colsum"][prev.name])
        else:
            own, rows = colsum_owner(qq, sh, mode, dev)
            got = b["colsum"][prev.name]
            assert got.numel() == rows * ref.shape[1], (l.name, got.numel(), rows, ref.shape)
            out[tag + "colsum"] = ratio(got.view(rows, ref.shape[1]), *_partials(ref, bound, own, rows))
    return out


def _colsum16(g16, got) -> float:
    """The colsum kernel's partial rows: f32 sums of ROWS_PER rows of the stored bf16 gradient."""
    M, N = g16.shape
    rows = -(-M // ROWS_PER)
    v = torch.zeros((rows * ROWS_PER, N), dtype=F64, device=g16.device)
    v[:M] = g16.double()
    v = v.view(rows, ROWS_PER, N)
    return ratio(got.view(rows, N), v.sum(1), (ROWS_PER + SLACK) * U * v.abs().sum(1))


# ------------------------------------------------- weight gradients, finalize ----
def check_grads(spec, b, pl, grads, slabs, loss, klw, only=None) -> dict:
    """``grads``: named arena gradients; ``slabs``: parameter name -> (tensor, rows) of the plan (weights with
    nsplit > 1 and every bias); ``loss``: the step's loss-history entry (None: not checked)."""
    M = b["z16"].shape[0]
    out = {}
    for i, l in enumerate(spec):
        if only is not None and l.name not in only:
            continue
        wp = pl[l.name]["W"]
        sh = shape_of(l, M)
        N, H, C, CO, k, s, p = sh
        numel = CO * k * k * C
        G, X = wg_pair(spec, i, b)
        ns = wp.nsplit
        slab = slabs[l.name + ".weight"][0] if ns > 1 else grads[l.name + ".weight"].reshape(-1)
        if ns > 1:
            assert slabs[l.name + ".weight"][1] == ns
        if wp.cfg == 110:
            x_f32 = X.dtype == torch.float32
            worst, total = dc.check_thin_wgrad(slab, X.reshape(M, H, H), G, x_f32)
            assert ns == M * ((H // 2) // 4)
        else:
            mps = wp.mt_per_split if wp.cfg < 100 else ((H // 2) ** 2) // 64
            worst, total = ck.check_wgrad(slab, sh, dict(G=G, X=X), ns, mps)
        out[f"WG.{l.name}.slabs"], out[f"WG.{l.name}.sum"] = worst, total
        sl = slab[:ns * numel].reshape(ns, numel).double()
        out[f"WG.{l.name}.weight"] = ratio(grads[l.name + ".weight"].reshape(numel), sl.sum(0),
                                           (ns + SLACK) * U * sl.abs().sum(0))
        t, r = slabs[l.name + ".bias"]
        rows = t.double().reshape(r, -1)
        assert rows.shape[1] == l.cout, (l.name, rows.shape)
        out[f"WG.{l.name}.bias"] = ratio(grads[l.name + ".bias"].reshape(-1), rows.sum(0),
                                         (r + SLACK) * U * rows.abs().sum(0))
    if loss is not None:
        bce, kld = b["bce_part"].double(), b["kld_part"].double()
        ref = bce.sum() + klw * kld.sum()
        bound = (bce.numel() + kld.numel() + SLACK) * U * (bce.abs().sum() + abs(klw) * kld.abs().sum())
        out["WG.loss"] = ratio(torch.tensor(float(loss), dtype=F64, device=ref.device), ref, bound)
    return out


def check_adam(spec, before, after, grads, hp, t) -> dict:
    """``before`` / ``after``: dict(params, exp_avg, exp_avg_sq[, w16]) of named tensors around the step;
    ``grads``: the finalized arena gradients; ``t``: the optimizer step (1-based)."""
    c = adam_consts(hp, t)
    out = {}
    for l in spec:
        for sfx in (".weight", ".bias"):
            n = l.name + sfx
            rp, rm, rv, bp, bm, bv = adam_ref(before["params"][n].reshape(-1), grads[n].reshape(-1),
                                              before["exp_avg"][n].reshape(-1), before["exp_avg_sq"][n].reshape(-1), c)
            out[f"AD.{n}.params"] = ratio(after["params"][n].reshape(-1), rp, bp)
            out[f"AD.{n}.exp_avg"] = ratio(after["exp_avg"][n].reshape(-1), rm, bm)
            out[f"AD.{n}.exp_avg_sq"] = ratio(after["exp_avg_sq"][n].reshape(-1), rv, bv)
            out[f"AD.{n}.w16"] = _bits_ratio(twin_ok(after["w16"][n].reshape(-1), after["params"][n].reshape(-1)))
    return out


def adam_hp(tr_hp: dict, decoupled: bool, schedule=None) -> dict:
    """The hyper-parameter dict ``adam_consts`` takes from a trainer's ``hp``."""
    return dict(lr=tr_hp["lr"], beta1=tr_hp["beta1"], beta2=tr_hp["beta2"], eps=tr_hp["eps"],
                weight_decay=tr_hp["weight_decay"], grad_scale=tr_hp["grad_scale"], decoupled=decoupled,
                lr_warmup_steps=getattr(schedule, "lr_warmup_steps", 0) if schedule is not None else 0)


# -------------------------------------------------------------------- stages ----
def stages(spec):
    """Stage names in step order."""
    enc = [l.name for l in spec if l.name.startswith("enc")]
    dec = [l.name for l in spec if l.name.startswith("dec")]
    return (["F.gather"] + ["F." + n for n in enc] + ["F.reparam"] + ["F." + n for n in dec]
            + ["B." + l.name for l in reversed(spec[1:])] + ["WG", "AD"])


def stage_of(key: str) -> str:
    p = key.split(".")
    return p[0] if p[0] in ("WG", "AD", "EM") else p[0] + "." + p[1]


def first_failure(spec, ratios: dict):
    """The first stage (in step order) with a ratio > 1, or None."""
    for st in stages(spec) + ["EM"]:   # EM: the weight average after the step (knob_cases.check_ema)
        if any(not r <= 1 for k, r in ratios.items() if stage_of(k) == st):
            return st
    return None


def input_conditions(spec, b, spread: bool) -> dict:
    """The conditions a case's stored buffers must meet (asserted on the CPU emulation and on the GPU run):
    finite values; every ReLU layer with active and inactive elements (1 % each; 10 % for ``spread``); both
    signs in every stored gradient; logits not all saturated (0.01 < |dlog16| < 0.99 somewhere); logvar
    in [-12, 6]."""
    out = {"finite": bool(torch.isfinite(b["mulv"]).all() and torch.isfinite(b["dlog16"].float()).all()
                          and torch.isfinite(b["dmulv"]).all())}
    lo = 0.10 if spread else 0.01
    for l in spec[:-1]:
        if l.relu:
            z = float((b["acts"][l.name].float() == 0).double().mean())
            out["zeros." + l.name] = lo <= z <= 1 - lo
    for name, g in list(b["gacts"].items()) + [("dlog16", b["dlog16"]), ("dmulv16", b["dmulv16"])]:
        g = g.float()
        out["signs." + name] = bool((g > 0).any() and (g < 0).any())
    d = b["dlog16"].float().abs()
    out["unsaturated"] = bool(((d > 0.01) & (d < 0.99)).any())
    lv = b["mulv"][:, b["mulv"].shape[1] // 2:]
    out["logvar"] = bool((lv >= -12).all() and (lv <= 6).all())
    return out
