"""tests/direct_checker.py is not vacuous (CPU): a plain f32 emulation of every
kernel family passes every check, and each of twelve deliberately wrong
emulations -- the ways these kernels can be subtly wrong -- fails at least one.
The emulations are torch f32 convolutions / matmuls on the operands as the
kernels read them; the MFMA single-channel forms are emulated with explicit
hi / lo / lo2 bf16 term splits. ``test_mutation_is_caught`` prints, per
mutation, the checks that caught it. The exact-data cases are also verified
here to be exactly representable at every partial-sum order."""
import pytest
import torch
import torch.nn.functional as F

from multidisttorch_amd.ops.conv_layout import nchw, nhwc, torch_weight
from tests import direct_cases as dc
from tests import direct_checker as dk
from tests import igemm_checker as ck


# ------------------------------------------------------------ direct conv ----
def emu_direct(name, N, inp, ep, mut=None):
    _, mode, H, C, CO = dc.DIRECT[name][:5]
    w = torch_weight(inp["w"].float())
    if mode == dc.CONV:
        x = nchw(inp["A"].float())
        if mut == "halo":          # right-hand padding column = its neighbour, upper half of the image only
            xp = F.pad(x, (1, 1, 1, 1))
            xp[:, :, 1:H // 2, -1] = xp[:, :, 1:H // 2, -2]
            y = F.conv2d(xp, w, None, 2, 0)
        else:
            if mut == "evenodd":   # tap (1, 2) reads the odd-column slot of tap (1, 3)
                w = w.clone()
                w[:, :, 1, 3] += w[:, :, 1, 2]
                w[:, :, 1, 2] = 0
            y = F.conv2d(x, w, None, 2, 1)
    else:
        g = nchw(inp["A"].float())
        y = F.conv_transpose2d(g, w, None, 2, 1)
        if mut == "class_taps":    # one parity class multiplies the taps of its row neighbour
            y2 = F.conv_transpose2d(g, w[:, :, [1, 0, 3, 2], :], None, 2, 1)
            y[:, :, 0::2, 0::2] = y2[:, :, 0::2, 0::2]
    v = nhwc(y).reshape(-1, y.shape[1])
    if ep["bias"]:
        v = v + inp["bias"]
    if ep["relu"]:
        v = torch.relu(v)
    if ep["mask"]:
        keep = inp["mask"].float() != 0 if mut == "mask_after_relu" else inp["mask"].float() > 0
        v = torch.where(keep, v, torch.zeros_like(v))
    oh, ncols, rows, RB = dk.direct_out_geom(name, N)
    cs = v.view(N * RB, rows * oh, ncols).sum(1)
    if mut == "colsum_row":
        cs = cs[[1, 0] + list(range(2, cs.shape[0]))]
    return dict(y32=v, y16=v.to(ck.BF), colsum=cs)


def check_direct(name, N, mut=None, exact=False):
    mode = dc.DIRECT[name][1]
    inp = dk.direct_inputs(name, N, seed=1, exact=exact)
    ep = dict(bias=True, relu=True, mask=True)
    out = emu_direct(name, N, inp, ep, mut)
    acc, mag = ck.fwd_acc(mode, dc.direct_shape(name, N), inp)
    ref, m = ck.epilogue(acc, mag, inp, **ep)
    K = 16 * dc.DIRECT[name][3] if mode == dc.CONV else 4 * dc.DIRECT[name][4]
    cref, cb, cnt = dk.direct_colsum_ref(out["y32"], name, N)
    res = {"y32 bound": ck.check_fwd(out["y32"], ref, m, K) <= 1, "bf16 twin": ck.twin_ok(out["y16"], out["y32"]),
           "column-sum rows": dk.ratio(out["colsum"], cref, cb) <= 1}
    if exact:
        assert dk.exact_fits(cnt * m.max())
        res["exact y32"] = dk.bits_equal(out["y32"], ref)
        res["exact column sums"] = dk.bits_equal(out["colsum"], cref)
    return res


# -------------------------------------------------------- weight gradients ----
def check_dwgrad(mut=None, exact=False):
    name, N = "DwL2", 2
    _, H, C, CO, _ = dc.DWGRAD[name]
    inp = dk.dwgrad_inputs(name, N, seed=2, exact=exact)
    cols = ck.im2col(inp["X"].float(), 4, 2, 1).view(N, -1, 16 * C)
    G = inp["G"].float().view(N, -1, CO)
    rows = torch.stack([G[n].T @ cols[n] for n in range(N)])
    if mut == "swap_images":
        rows = rows[[1, 0]]
    out = rows.reshape(-1)
    worst, total = dk.check_dwgrad(out, name, N, inp)
    res = {"per-image rows": worst <= 1, "row sum": total <= 1}
    if exact:
        slabs, _ = ck.wgrad_ref(dk.dwgrad_shape(name, N), inp, (H // 2) ** 2 // 64)
        res["exact rows"] = all(dk.bits_equal(rows[i], r) for i, (r, _) in enumerate(slabs))
    return res


def emu_thin_wgrad(x, G, x_f32, shift=0):
    N, H, W = x.shape
    cols = ck.im2col(x.float().unsqueeze(-1), 4, 2, 1)
    terms = dk.split3(cols) if x_f32 else (cols,)
    Gm = G.float().reshape(-1, 32)
    rows = []
    for r0 in range(0, Gm.shape[0], 256):
        sl = slice(r0 + 64 * shift, r0 + 64 * shift + 256)
        rows.append(sum(Gm[sl].T @ t[sl] for t in terms))
    return torch.stack(rows).reshape(-1)


def check_thin_wgrad(x_f32, mut=None, exact=False):
    g = (2, 16, 128)
    if exact:
        x, G, unit = dk.exact_thin_wgrad(x_f32, g, seed=4)
    else:
        inp = dk.thin_inputs(32, g, x_f32, seed=3)
        x, G = inp["x"], inp["G"]
    out = emu_thin_wgrad(x, G, x_f32, shift=1 if mut == "shifted_rows" else 0)
    worst, total = dk.check_thin_wgrad(out, x, G, x_f32)
    res = {"per-block rows": worst <= 1, "row sum": total <= 1}
    if exact:
        slabs, _ = dk.thin_wgrad_refs(x, G, x_f32)
        res["exact rows"] = all(dk.bits_equal(out.view(-1, 32, 16)[i], r) for i, (r, _) in enumerate(slabs))
    return res


# --------------------------------------------------------------- thin_conv ----
def emu_thin_conv(x, w, bias, relu, mask, mfma, mut=None):
    CO = w.shape[0]
    cols = ck.im2col(x.float().unsqueeze(-1), 4, 2, 1)
    wm = w.view(CO, 16)
    if mfma:    # (Wh + Wl + Wl2)(xh + xl) + Wh xl2, the small terms first
        xh, xl, xl2 = dk.split3(cols)
        wh, wl, wl2 = dk.split3(wm)
        acc = torch.zeros(cols.shape[0], CO)
        if mut != "w_two_terms":
            acc = acc + xl @ wl2.T + xh @ wl2.T
        acc = acc + xl @ wl.T + xh @ wl.T
        if mut != "x_two_terms":
            acc = acc + xl2 @ wh.T
        acc = acc + xl @ wh.T + xh @ wh.T
    else:
        acc = cols @ wm.T
    v = acc + bias if bias is not None else acc
    if relu:
        v = torch.relu(v)
    if mask is not None:
        v = torch.where(mask.float() > 0, v, torch.zeros_like(v))
    M = v.shape[0]
    nb = -(-M // 256)
    cs = F.pad(v, (0, 0, 0, nb * 256 - M)).view(nb, 256, CO).sum(1)
    return v.to(ck.BF), cs


def check_thin_conv(CO, g, x_f32, kind=None, mut=None):
    mfma = dc.thin_mfma_geom(CO, g)
    inp = dk.thin_inputs(CO, g, x_f32, seed=5)
    unit = None
    if kind:
        x, w, bias, unit = dk.exact_thin_conv(kind, CO, g, seed=2)
    else:
        x, w, bias = inp["x"], inp["w"], inp["bias"]
    y16, cs = emu_thin_conv(x, w, bias, False, inp["mask"], mfma, mut)
    acc, mag = dk.thin_conv_acc(x, w)
    ref, m = dk.thin_epilogue(acc, mag, bias, False, inp["mask"])
    b = dk.thin_conv_bound(m, CO, g)
    cref, cb = dk.thin_colsum_ref(ref, b)
    res = {"y16 bound": dk.y16_ratio(y16, ref, b) <= 1, "column-sum rows": dk.ratio(cs, cref, cb) <= 1}
    if kind:
        cmag, _ = dk.thin_colsum_ref(m, m)
        assert dk.exact_fits(1.02 * m, unit) and dk.exact_fits(1.02 * cmag, unit)
        res["exact column sums"] = dk.bits_equal(cs, cref)
        res["exact y16"] = torch.equal(y16, ref.to(ck.BF))
    return res


# -------------------------------------------------------------- thin_tconv ----
def emu_thin_tconv(G, w, bias, tgt, CO, g, mut=None):
    N, H, W = g
    gg = nchw(G.float())
    wt = w.view(CO, 1, 4, 4)
    if dc.tconv_patch_geom(CO, g):
        hi, lo, lo2 = dk.split3(wt)
        t = F.conv_transpose2d(gg, lo2, None, 2, 1) + F.conv_transpose2d(gg, lo, None, 2, 1)
        t = (t + F.conv_transpose2d(gg, hi, None, 2, 1) + bias).view(N, H, W)
    else:
        t = F.conv_transpose2d(gg, wt, bias, 2, 1).view(N, H, W)
    x = tgt
    p = 1 / (1 + torch.exp(-t))
    sp = torch.log1p(torch.exp(t)) if mut == "softplus" else torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    if mut == "no_clamp":
        loss = x * (sp - t) + (1 - x) * sp
    else:
        loss = x * torch.clamp(sp - t, max=100.0) + (1 - x) * torch.clamp(sp, max=100.0)
    gr = p - x
    owners = dk.tconv_owners(CO, g)
    part = torch.stack([loss.reshape(-1)[o].sum() for o in owners])
    gpart = torch.stack([gr.reshape(-1)[o].sum() for o in owners])
    if mut == "dead_lanes":   # the tail block's dead lanes (clamped to class pixel 0) are added as well
        for c in range(4):
            last = len(owners) // 4 * (c + 1) - 1
            dead = 256 - owners[last].numel()
            part[last] += dead * loss.reshape(-1)[owners[last - (len(owners) // 4 - 1)][0]]
    return dict(y32=t.reshape(-1), dlog16=gr.to(ck.BF).reshape(-1), recon=p.reshape(-1), part=part, gpart=gpart)


def check_thin_tconv(CO, g, saturated=False, kind=None, mut=None):
    N, H, W = g
    inp = dk.thin_inputs(CO, g, True, seed=6)
    G, w, bias = inp["G"], inp["tw"], inp["tbias"]
    if kind:
        G, w, bias, unit = dk.exact_thin_tconv(kind, CO, g, seed=3)
    if saturated:
        w = dk.saturate(w, G, H, W, bias)
    out = emu_thin_tconv(G, w, bias, inp["tgt"], CO, g, mut)
    t, mag = dk.thin_tconv_acc(G, w, H, W, bias)
    b_t = dk.thin_tconv_bound(mag, CO, g)
    res = {"logits bound": dk.ratio(out["y32"].view(t.shape), t, b_t) <= 1}
    res.update({f"{k} bound": r <= 1 for k, r in dk.check_bce(out, t, b_t, inp["tgt"], dk.tconv_owners(CO, g)).items()})
    if saturated:
        assert float(t.min()) <= -150 and float(t.max()) >= 150
        res["finite"] = all(bool(torch.isfinite(v.float()).all()) for v in out.values())
        res["recon exactly 0 / 1"] = dk.saturated_recon_ok(out["recon"], t)
    if kind:
        assert dk.exact_fits(1.02 * mag, unit)
        res["exact logits"] = dk.bits_equal(out["y32"].view(t.shape), t)
    return res


# --------------------------------------------------------------------------------
MFMA_G, VALU_G, PATCH_G = (3, 16, 128), (2, 28, 28), (1, 128, 128)

FAMILIES = {
    "direct conv DcS2": lambda m=None: check_direct("DcS2", 1, m),
    "direct conv DcS3 (one row block)": lambda m=None: check_direct("DcS3", 2, m),
    "direct tconv DcT2": lambda m=None: check_direct("DcT2", 1, m),
    "direct conv exact": lambda m=None: check_direct("DcS2", 1, m, exact=True),
    "direct tconv exact": lambda m=None: check_direct("DcT1", 2, m, exact=True),
    "dwgrad": check_dwgrad,
    "dwgrad exact": lambda m=None: check_dwgrad(m, exact=True),
    "thin_wgrad f32": lambda m=None: check_thin_wgrad(True, m),
    "thin_wgrad bf16": lambda m=None: check_thin_wgrad(False, m),
    "thin_wgrad f32 exact": lambda m=None: check_thin_wgrad(True, m, exact=True),
    "thin_wgrad bf16 exact": lambda m=None: check_thin_wgrad(False, m, exact=True),
    "thin_conv VALU f32": lambda m=None: check_thin_conv(16, VALU_G, True, None, m),
    "thin_conv VALU bf16": lambda m=None: check_thin_conv(64, VALU_G, False, None, m),
    "thin_conv VALU exact": lambda m=None: check_thin_conv(32, (3, 10, 14), True, "ints", m),
    "thin_conv MFMA f32": lambda m=None: check_thin_conv(32, MFMA_G, True, None, m),
    "thin_conv MFMA bf16": lambda m=None: check_thin_conv(32, MFMA_G, False, None, m),
    "thin_conv MFMA exact (a)": lambda m=None: check_thin_conv(32, MFMA_G, True, "x3", m),
    "thin_conv MFMA exact (b)": lambda m=None: check_thin_conv(32, MFMA_G, True, "w3", m),
    "thin_tconv VALU": lambda m=None: check_thin_tconv(32, VALU_G, mut=m),
    "thin_tconv VALU odd": lambda m=None: check_thin_tconv(16, (3, 10, 14), mut=m),
    "thin_tconv VALU saturated": lambda m=None: check_thin_tconv(32, VALU_G, saturated=True, mut=m),
    "thin_tconv VALU exact": lambda m=None: check_thin_tconv(64, (3, 10, 14), kind="ints", mut=m),
    "thin_tconv patch": lambda m=None: check_thin_tconv(32, PATCH_G, mut=m),
    "thin_tconv patch saturated": lambda m=None: check_thin_tconv(32, PATCH_G, saturated=True, mut=m),
    "thin_tconv patch exact": lambda m=None: check_thin_tconv(32, PATCH_G, kind="w3", mut=m),
}

# mutation -> (family it is applied to, the check that must catch it, its argument)
MUTATIONS = {
    "right-hand halo column read as the neighbour on one edge": ("direct conv DcS2", "y32 bound", "halo"),
    "even and odd patch columns swapped for one tap": ("direct conv DcS2", "y32 bound", "evenodd"),
    "one parity class uses another class's taps": ("direct tconv DcT2", "y32 bound", "class_taps"),
    "column-sum row stored under the neighbouring row block": ("direct conv DcS2", "column-sum rows", "colsum_row"),
    "two images' weight-gradient rows swapped": ("dwgrad", "per-image rows", "swap_images"),
    "thin_wgrad row covers rows shifted by one": ("thin_wgrad bf16", "per-block rows", "shifted_rows"),
    "mask applied after ReLU keeps a value it should zero": ("direct conv DcS2", "y32 bound", "mask_after_relu"),
    "two-term input split in the MFMA thin_conv": ("thin_conv MFMA exact (a)", "exact column sums", "x_two_terms"),
    "two-term weight split in the MFMA thin_conv": ("thin_conv MFMA exact (b)", "exact column sums", "w_two_terms"),
    "BCE without the clamp": ("thin_tconv VALU saturated", "part bound", "no_clamp"),
    "softplus as log1p(exp(t))": ("thin_tconv VALU saturated", "part bound", "softplus"),
    "part[bid] includes the tail block's dead lanes": ("thin_tconv VALU", "part bound", "dead_lanes"),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_f32_emulation_passes_every_check(family):
    res = FAMILIES[family]()
    assert res and all(res.values()), {k: v for k, v in res.items() if not v}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutation_is_caught(mutation):
    family, check, arg = MUTATIONS[mutation]
    res = FAMILIES[family](arg)
    caught = [k for k, v in res.items() if not v]
    print(f"{mutation} [{family}]: caught by {caught}")
    assert check in caught, (mutation, res)


def test_swapped_rows_keep_the_totals():
    """The two mutations that permute partial rows are invisible to a check of the total alone."""
    assert check_dwgrad("swap_images")["row sum"]
    inp = dk.direct_inputs("DcS2", 1, seed=1)
    ep = dict(bias=True, relu=True, mask=True)
    a, b = emu_direct("DcS2", 1, inp, ep), emu_direct("DcS2", 1, inp, ep, "colsum_row")
    assert torch.equal(a["colsum"].double().sum(0), b["colsum"].double().sum(0))
    assert not torch.equal(a["colsum"], b["colsum"])


def test_needs3_data_needs_all_three_terms():
    v = dk.needs3((64, 16), 1)
    assert dk.terms_nonzero(v)
    hi, lo, lo2 = dk.split3(v)
    assert bool((hi + lo != v).all())           # two terms are not enough
    assert not dk.terms_nonzero(torch.tensor([0.5, 0.75]))


def test_exact_cases_are_representable_in_any_order():
    """sum|terms| of every exact case stays below 2^24 units of the last place."""
    for name in dc.DIRECT:
        inp = dk.direct_inputs(name, 1, seed=7, exact=True)
        _, mag = ck.fwd_acc(dc.DIRECT[name][1], dc.direct_shape(name, 1), inp)
        oh, _, rows, _ = dk.direct_out_geom(name, 1)
        assert dk.exact_fits((mag.max() + 3) * rows * oh)
    # ... and at any N and seed by construction: K + 3 per element, times the pixels of a column-sum row
    for name, v in dc.DIRECT.items():
        K = 16 * v[3] if v[1] == dc.CONV else 4 * v[4]
        oh, _, rows, _ = dk.direct_out_geom(name, 1)
        assert (K + 3) * rows * oh < 2 ** 24
    for name, (_, H, C, CO, _) in dc.DWGRAD.items():
        assert max(dc.DWGRAD_N) * (H // 2) ** 2 < 2 ** 24
    for g in dc.THIN_WGRAD:
        x, G, unit = dk.exact_thin_wgrad(True, g, seed=4)
        Ga, ca = G.double().abs().reshape(-1, 32), ck.im2col(x.double().unsqueeze(-1), 4, 2, 1)
        assert dk.terms_nonzero(x)
        assert all(dk.exact_fits(1.02 * (Ga[r:r + 256].T @ ca[r:r + 256]), unit) for r in range(0, Ga.shape[0], 256))
    for kind in ("x3", "w3"):
        for _, g in dc.THIN_CONV_MFMA:
            x, w, bias, unit = dk.exact_thin_conv(kind, 32, g, seed=2)
            _, mag = dk.thin_conv_acc(x, w)
            cmag, _ = dk.thin_colsum_ref(mag, mag)
            assert dk.terms_nonzero(x if kind == "x3" else w) and dk.exact_fits(1.02 * cmag, unit)
    G, w, bias, unit = dk.exact_thin_tconv("w3", 32, PATCH_G, seed=3)
    _, mag = dk.thin_tconv_acc(G, w, 128, 128, bias)
    assert dk.terms_nonzero(w) and dk.exact_fits(1.02 * mag, unit)


def test_half_ulp_and_y16_ratio():
    v = torch.tensor([1.0, 1.5, 255.0, 0.0, 3.0e-3], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 0.5, dk.TINY, 2.0 ** -17], dtype=torch.float64)
    assert torch.equal(dk.half_ulp_bf16(v), want)
    ref = torch.tensor([1.00390625], dtype=torch.float64)            # halfway between two bf16 values
    zero = torch.zeros(1, dtype=torch.float64)
    assert dk.y16_ratio(torch.tensor([1.0], dtype=ck.BF), ref, zero) <= 1
    assert dk.y16_ratio(torch.tensor([1.015625], dtype=ck.BF), ref, zero) > 1


def test_block_maps_partition_the_pixels():
    for CO, g in dc.THIN_TCONV_VALU + dc.THIN_TCONV_PATCH:
        own = dk.tconv_owners(CO, g)
        assert len(own) == dc.thin_tconv_blocks(CO, g)
        allpx = torch.cat(own)
        assert allpx.numel() == g[0] * g[1] * g[2] == allpx.unique().numel()
    # class 0 = (ca, cb) = (0, 0) holds the odd rows and odd columns
    o = dk.tconv_valu_owners(1, 4, 6)[0]
    assert o.tolist() == [7, 9, 11, 19, 21, 23]
