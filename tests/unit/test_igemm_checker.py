"""The checker of the conv GEMM tile tests (tests/igemm_checker.py) is not
vacuous. (a) Its float64 oracles agree with torch's own float64 conv,
transposed conv and conv weight gradient, and its parity-row map with a
brute-force enumeration. (b) A plain f32 torch emulation of each kernel passes
every bound at reduced-row versions of the GPU test's cases, and each mutated
emulation (a bug the norm-relative criterion of test_conv_igemm.py could let
through) fails it. Mutants live in these emulations only; no mutated kernel
exists."""
import pytest
import torch
import torch.nn.functional as F

from multidisttorch_amd.ops.conv_layout import nchw, nhwc, torch_weight
from tests import igemm_cases as cs
from tests import igemm_checker as ck

F32, F64 = torch.float32, torch.float64
FWD = [(n, m, t, c, cs.reduced(sh)) for n, m, t, c, sh in cs.fwd_cases()]
FWD_IDS = [c[0] for c in FWD]


def _a32(inp):
    return inp["A"].to(ck.BF).to(F32)


# ------------------------------------------------------- f32 emulations ----
def emu_acc(mode, shape, inp, mut=None):
    """[rows, Ncols] f32 accumulators in the output's NHWC order: conv mode as
    the im2col matmul, parity mode through torch's own transposed conv."""
    N, H, C, CO, k, s, p = shape
    a, w = _a32(inp), inp["w"].to(F32)
    if mode == cs.PARITY:
        assert mut is None
        return nhwc(F.conv_transpose2d(nchw(a), torch_weight(w), None, s, p)).reshape(-1, C)
    cols, wm = ck.im2col(a, k, s, p), w.reshape(CO, -1)
    K = cols.shape[1]
    if mut == "drop_last_k_chunk":      # the partial last k-tile never staged
        assert K % 64
        cols = cols[:, :K - K % 64]
        wm = wm[:, :K - K % 64]
    acc = cols @ wm.T
    if mut == "drop_chunk_one_row":     # one 16-B chunk of one row zeroed at the LDS store
        r = cols.shape[0] - 1
        acc[r] -= cols[r, 8:16] @ wm[:, 8:16].T
    return acc


def emu_fwd(mode, shape, inp, BM, BN, bias=False, relu=False, mask=False, mut=None):
    """(y32 [rows, Ncols], colsum [classes mtiles, Ncols]) in f32."""
    classes, M, Ncols, K = cs.fwd_geom(mode, shape)
    acc = emu_acc(mode, shape, inp, mut if mut in ("drop_last_k_chunk", "drop_chunk_one_row") else None)
    b = inp["bias"].clone() if bias else torch.zeros(Ncols)
    if mut == "bias_shift":             # the last column tile reads the previous tile's bias
        c0 = (-(-Ncols // BN) - 1) * BN
        assert c0 >= BN
        b[c0:] = inp["bias"][c0 - BN:Ncols - BN]
    v = acc + b
    if relu:
        v = torch.relu(acc) + b if mut == "relu_before_bias" else torch.relu(v)
    rows = ck.class_rows(mode, shape)
    m = inp["mask"].to(F32) if mask else torch.ones_like(v)
    if mut == "mask_wrong_class":       # class c masked with the pixels of class c + 1
        assert classes > 1
        m2 = m.clone()
        for c in range(classes):
            m2[rows[c]] = m[rows[(c + 1) % classes]]
        m = m2
    y = torch.where(m > 0, v, torch.zeros_like(v))
    mtiles = -(-M // BM)
    csum = torch.zeros(classes * mtiles, Ncols)
    for c in range(classes):
        yc, vc = y[rows[c]], v[rows[c]]
        for mt in range(mtiles):
            t = yc[mt * BM:(mt + 1) * BM].sum(0)
            if mut == "colsum_masked_row":   # the first row of every tile summed before its mask
                t = t - yc[mt * BM] + vc[mt * BM]
            if mut == "colsum_rows_ge_M" and mt == mtiles - 1:
                # rows >= M summed: their gathers are clamped to row 0, so they hold row 0's value
                t = t + (mtiles * BM - M) * yc[0]
            csum[c * mtiles + mt] = t
    return y, csum


def emu_wgrad(shape, inp, mps, mut=None):
    """[nsplit, CO, K2] f32 partial slabs."""
    N, H, C, CO, k, s, p = shape
    cols = ck.im2col(inp["X"].to(ck.BF).to(F32), k, s, p)
    G = inp["G"].to(F32).reshape(-1, CO)
    M, step = G.shape[0], 64 * mps
    bounds = list(range(0, M, step)) + [M]
    if mut == "tile_to_neighbour":      # the last m-tile of split 0 summed into split 1
        bounds[1] -= 64
    return torch.stack([G[a:b].T @ cols[a:b] for a, b in zip(bounds[:-1], bounds[1:])])


# ----------------------------------------------- (a) oracles vs torch f64 ----
@pytest.mark.parametrize("shape", [(2, 14, 8, 24, 4, 2, 1), (3, 9, 3, 8, 3, 1, 1), (7, 1, 72, 8, 1, 1, 0)])
def test_oracles_agree_with_torch_float64(shape):
    N, H, C, CO, k, s, p = shape
    inp = ck.fwd_inputs(cs.CONV, shape, seed=1)
    x, w = inp["A"].to(F64), inp["w"].to(F64)
    want = nhwc(F.conv2d(nchw(x), torch_weight(w), None, s, p)).reshape(-1, CO)
    torch.testing.assert_close(ck.conv_ref(x, w, s, p), want, rtol=1e-12, atol=1e-12)
    # k-ranges partition the sum
    K = k * k * C
    parts = ck.conv_ref(x, w, s, p, 0, K // 2) + ck.conv_ref(x, w, s, p, K // 2, K)
    torch.testing.assert_close(parts, want, rtol=1e-12, atol=1e-12)
    wi = ck.wgrad_inputs(shape, seed=2)
    _, full = ck.wgrad_ref(shape, wi, 1)
    gw = torch.nn.grad.conv2d_weight(nchw(wi["X"].to(F64)), (CO, C, k, k), nchw(wi["G"].to(F64)), s, p)
    torch.testing.assert_close(full, gw.permute(0, 2, 3, 1).reshape(CO, -1), rtol=1e-12, atol=1e-12)
    if (H + 2 * p - k) % s == 0:   # the conv's backward-data reproduces the input extent
        pi = ck.fwd_inputs(cs.PARITY, shape, seed=3)
        g, wp = pi["A"].to(F64), pi["w"].to(F64)
        want = nhwc(F.conv_transpose2d(nchw(g), torch_weight(wp), None, s, p)).reshape(-1, C)
        torch.testing.assert_close(ck.tconv_ref(g, wp, s, p, H), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", [(2, 6, 8, 8, 4, 2, 1), (3, 14, 8, 24, 4, 2, 1), (2, 4, 8, 8, 2, 2, 0)])
def test_parity_rows_against_brute_force(shape):
    N, H, C, CO, k, s, p = shape
    seen = []
    for cls in range(s * s):
        ca, cb = divmod(cls, s)
        want = [(n * H + iy) * H + ix for n in range(N) for iy in range(H) for ix in range(H)
                if (iy + p) % s == ca and (ix + p) % s == cb]
        got = ck.parity_rows(shape, cls).tolist()
        assert got == want      # same pixels, in row order (n, yy, xx)
        seen += got
    assert sorted(seen) == list(range(N * H * H))


def test_mask_has_both_signs_and_exact_zeros():
    m = ck.fwd_inputs(cs.PARITY, (3, 14, 8, 24, 4, 2, 1))["mask"].float()
    assert bool((m > 0).any()) and bool((m < 0).any()) and bool((m == 0).any())


# ------------------------------------- (b) emulations against the bounds ----
@pytest.mark.parametrize("name,mode,thin,cfg,shape", FWD, ids=FWD_IDS)
def test_f32_emulation_passes_forward_bounds(name, mode, thin, cfg, shape):
    BM, BN = cs.FWD_TILES[cfg]
    K = cs.fwd_geom(mode, shape)[3]
    for a_f32 in ((True, False) if thin else (False,)):
        inp = ck.fwd_inputs(mode, shape, a_f32=a_f32, seed=cfg)
        for ep in (dict(bias=True, relu=True), dict(mask=True)):
            y, csum = emu_fwd(mode, shape, inp, BM, BN, **ep)
            ref, mag = ck.fwd_ref(mode, shape, inp, **ep)
            assert ck.check_fwd(y, ref, mag, K) <= 1
            cref, cb = ck.colsum_ref(y, mode, shape, BM)
            assert ck.ratio(csum, cref, cb) <= 1


LIN = cs.reduced(cs.FWD_CONV_VEC[2][1])      # F1 Linear form, K = 136
SPAT = cs.reduced(cs.FWD_CONV_VEC[3][1])     # F1 4x4 form
PAR = cs.reduced(cs.FWD_PARITY[1][1])        # parity F1


@pytest.mark.parametrize("mut,mode,shape,ep", [
    ("drop_last_k_chunk", cs.CONV, LIN, dict(bias=True, relu=True)),
    ("drop_chunk_one_row", cs.CONV, LIN, dict(bias=True, relu=True)),
    ("drop_chunk_one_row", cs.CONV, SPAT, dict(mask=True)),
    ("bias_shift", cs.CONV, LIN, dict(bias=True, relu=True)),
    ("bias_shift", cs.PARITY, PAR, dict(bias=True, relu=True)),
    ("relu_before_bias", cs.CONV, SPAT, dict(bias=True, relu=True)),
    ("mask_wrong_class", cs.PARITY, PAR, dict(mask=True)),
])
def test_mutated_forward_emulations_fail(mut, mode, shape, ep):
    BM, BN = cs.FWD_TILES[1]
    K = cs.fwd_geom(mode, shape)[3]
    inp = ck.fwd_inputs(mode, shape, seed=5)
    ref, mag = ck.fwd_ref(mode, shape, inp, **ep)
    assert ck.check_fwd(emu_fwd(mode, shape, inp, BM, BN, **ep)[0], ref, mag, K) <= 1
    assert ck.check_fwd(emu_fwd(mode, shape, inp, BM, BN, mut=mut, **ep)[0], ref, mag, K) > 1


@pytest.mark.parametrize("mode,shape", [(cs.CONV, SPAT), (cs.PARITY, PAR)])
@pytest.mark.parametrize("mut", ["colsum_masked_row", "colsum_rows_ge_M"])
def test_mutated_column_sums_fail(mut, mode, shape):
    BM, BN = cs.FWD_TILES[1]
    assert cs.fwd_geom(mode, shape)[1] % BM
    inp = ck.fwd_inputs(mode, shape, seed=6)
    y, csum = emu_fwd(mode, shape, inp, BM, BN, mask=True, mut=mut)
    cref, cb = ck.colsum_ref(y, mode, shape, BM)
    assert ck.ratio(emu_fwd(mode, shape, inp, BM, BN, mask=True)[1], cref, cb) <= 1
    assert ck.ratio(csum, cref, cb) > 1


@pytest.mark.parametrize("cfg,ktiles,shape", cs.SPLITK)
def test_splitk_emulation_and_dropped_slab(cfg, ktiles, shape):
    N, H, C, CO, k, s, p = shape
    inp = ck.fwd_inputs(cs.CONV, shape, seed=7)
    kps = 4 if ktiles == 18 else 1          # a ragged split: 18 k-tiles in 5 slabs, the last of 2
    a, w = _a32(inp).reshape(N, C), inp["w"].to(F32).reshape(CO, C)
    refs = ck.slab_refs(shape, inp, ktiles, kps)
    slabs = [a[:, 64 * t:64 * (t + kps)] @ w[:, 64 * t:64 * (t + kps)].T for t in range(0, ktiles, kps)]
    assert len(refs) == len(slabs) == -(-ktiles // kps)
    assert max(ck.ratio(z, r, b) for z, (r, b) in zip(slabs, refs)) <= 1
    ref, mag = ck.fwd_ref(cs.CONV, shape, inp, bias=True, relu=True)
    y = torch.relu(torch.stack(slabs).sum(0) + inp["bias"])
    assert ck.check_fwd(y, ref, mag, C, len(slabs)) <= 1
    y = torch.relu(torch.stack(slabs[:-1]).sum(0) + inp["bias"])
    assert ck.check_fwd(y, ref, mag, C, len(slabs)) > 1
    # a slab that summed the neighbouring k-tile fails its own check
    assert ck.ratio(slabs[1], *refs[0]) > 1


WG = [(n, t, f, c, sh, 3 if sh[0] == 40 else 2) for n, t, f, c, sh in cs.wgrad_cases()]


@pytest.mark.parametrize("name,thin,x_f32,cfg,shape,mps", WG, ids=[c[0] for c in WG])
def test_wgrad_emulation_and_moved_tile(name, thin, x_f32, cfg, shape, mps):
    inp = ck.wgrad_inputs(shape, x_f32=x_f32, seed=cfg)
    out = emu_wgrad(shape, inp, mps)
    ns = out.shape[0]
    assert ns >= 2
    worst, total = ck.check_wgrad(out.flatten(), shape, inp, ns, mps)
    assert worst <= 1 and total <= 1
    worst, total = ck.check_wgrad(emu_wgrad(shape, inp, mps, "tile_to_neighbour").flatten(), shape, inp, ns, mps)
    assert worst > 1 and total <= 1     # only the per-slab check sees a tile in the wrong split


def test_sentinels_see_overruns_and_unwritten_elements():
    for dt in (torch.float32, ck.BF):
        t = ck.guarded(100, dt)
        assert t.numel() == 100 + ck.GUARD and ck.untouched(t) and not ck.written(t, 100)
        t[:100] = 1.0
        assert ck.written(t, 100) and ck.untouched(t, 100)
        t[57] = ck._fill(dt)
        assert not ck.written(t, 100)           # an unwritten tail element
        t[57] = 1.0
        t[100] = 0.0
        assert not ck.written(t, 100)           # a write past the row or column tail
    a = torch.tensor([1.0, 1.00390625, -3.0])
    assert ck.twin_ok(a.to(ck.BF), a) and not ck.twin_ok(torch.tensor([1.0, 1.0078125, -3.0]).to(ck.BF), a)
