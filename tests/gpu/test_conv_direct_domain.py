"""The direct and single-channel conv kernels per element against float64
oracles: the six patch-resident direct convs (conv_direct.h), the direct weight
gradient (conv_dwgrad.h), thin_conv / thin_tconv in their VALU, MFMA and
halo-patch forms and thin_wgrad_k (conv_thin.h, conv_thin_wg.h).

Cases come from tests/direct_cases.py, oracles, bounds and block maps from
tests/direct_checker.py (whose docstring derives every bound; none is
measured). Every output is a poisoned, guarded buffer; every result is printed
as an error/bound ratio and must be <= 1; bf16 twins, optional-output
combinations, the gather form and the job forms are compared bit for bit; the
exact-data cases must equal the oracle bit for bit. The switches that select
other kernel bodies are read once per process, so only the default forms run
here (a non-default environment skips)."""
import os

import pytest
import torch

from multidisttorch_amd.ops import conv_plans as plans
from tests import direct_cases as dc
from tests import direct_checker as dk
from tests import igemm_cases as ics
from tests import igemm_checker as ck

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True)
def _default_forms():
    bad = dc.non_default_env(os.environ)
    if bad:
        pytest.skip(f"non-default kernel switches in the environment: {bad}")


def _ok(tag, r):
    print(f"{tag}: error/bound {r:.4f}")
    assert r <= 1, f"{tag}: error/bound {r}"


# ------------------------------------------------------------- direct conv ----
def _plan(C, name, N, fwd=True):
    cfg, mode, H, Ci, CO, BM, BN, R, per_img = dc.DIRECT[name]
    q = plans.igemm_plan(mode, dc.desc(N, H, H, Ci, CO), False, fwd=fwd)
    assert q.cfg == cfg and (q.bm, q.bn) == (BM, BN) and q.mtiles * q.ntiles == per_img * N, q
    return dict(mode=mode, d=dc.desc(N, H, H, Ci, CO), n=q.classes * q.m * q.ncols, ncols=q.ncols, K=q.k, rows=q.colsum_rows)


def _launch_direct(C, q, inp, ep, job=None, fwd=True):
    out = dict(y16=ck.guarded(q["n"], ck.BF, DEV) if ep["y16"] else None,
               y32=ck.guarded(q["n"], device=DEV) if ep["y32"] else None,
               colsum=ck.guarded(q["rows"] * q["ncols"], device=DEV) if ep["colsum"] else None)
    kw = dict(job=job) if job is not None else dict(fwd=fwd)
    C.igemm(q["mode"], inp["A"], inp["B16"], q["d"], inp["bias"] if ep["bias"] else None, ep["relu"], out["y16"],
            out["y32"], inp["mask"].flatten() if ep["mask"] else None, out["colsum"], **kw)
    return out


def _check_direct(tag, name, N, q, inp, ep, out, acc, mag, exact=False):
    n = q["n"]
    for k, v in out.items():
        if v is not None:
            assert ck.written(v, q["rows"] * q["ncols"] if k == "colsum" else n), f"{tag}: {k} unwritten or overrun"
    assert ck.twin_ok(out["y16"][:n], out["y32"][:n]), f"{tag}: y16 is not the bf16 rounding of y32"
    ref, m = ck.epilogue(acc, mag, inp, bias=ep["bias"], relu=ep["relu"], mask=ep["mask"])
    if exact:
        assert dk.exact_fits(m) and dk.bits_equal(out["y32"][:n], ref), f"{tag}: y32 differs from the exact oracle"
    else:
        _ok(tag, ck.check_fwd(out["y32"][:n], ref, m, q["K"]))
    if out["colsum"] is not None:
        cref, cb, cnt = dk.direct_colsum_ref(out["y32"][:n], name, N)
        got = out["colsum"][:cref.numel()].view(cref.shape)
        if exact:
            assert dk.exact_fits(cnt * m.max()) and dk.bits_equal(got, cref), f"{tag}: column sums not exact"
        else:
            _ok(f"{tag} column sums", dk.ratio(got, cref, cb))


@pytest.mark.parametrize("N", dc.DIRECT_N)
@pytest.mark.parametrize("name", list(dc.DIRECT))
def test_direct_conv(name, N, native_ext):
    C = native_ext
    q = _plan(C, name, N)
    inp = dk.direct_inputs(name, N, seed=N, device=DEV)
    acc, mag = ck.fwd_acc(q["mode"], dc.direct_shape(name, N), inp)
    both = dict(dc.DIRECT_EPILOGUES["all_y16"], y32=True)
    for en, ep in dc.DIRECT_EPILOGUES.items():
        tag = f"{name} N={N} {en}"
        if en == "all_y16":   # the trainer's call: y16 alone must be the bits of the launch that stores both
            full = _launch_direct(C, q, inp, both)
            _check_direct(tag + " (with y32)", name, N, q, inp, both, full, acc, mag)
            out = _launch_direct(C, q, inp, ep)
            assert ck.same_bits(out["y16"], full["y16"]) and ck.same_bits(out["colsum"], full["colsum"]), tag
        elif en == "plain_y32":
            out = _launch_direct(C, q, inp, ep)
            assert ck.written(out["y32"], q["n"]), tag
            _ok(tag, ck.check_fwd(out["y32"][:q["n"]], acc, mag, q["K"]))
        else:
            _check_direct(tag, name, N, q, inp, ep, _launch_direct(C, q, inp, ep), acc, mag)


@pytest.mark.parametrize("name", list(dc.DIRECT))
def test_direct_conv_exact(name, native_ext):
    """{-1, 0, 1} operands and an integer bias: y32 and the column sums equal the oracle bit for bit."""
    C = native_ext
    q = _plan(C, name, 3)
    inp = dk.direct_inputs(name, 3, seed=7, device=DEV, exact=True)
    acc, mag = ck.fwd_acc(q["mode"], dc.direct_shape(name, 3), inp)
    ep = dict(dc.DIRECT_EPILOGUES["all_y16"], y32=True)
    _check_direct(f"{name} exact", name, 3, q, inp, ep, _launch_direct(C, q, inp, ep), acc, mag, exact=True)


@pytest.mark.parametrize("name", list(dc.DIRECT_JOBS))
def test_direct_job_form_is_bitwise(name, native_ext):
    """The direct body recorded as a job (backward-data call) next to a W0
    weight-gradient job: where conv_jobs.hip kCombos has the pair, one fused
    launch stores exactly what the stand-alone launches store, guards included;
    where it has not, launch_jobs refuses and nothing is written."""
    C = native_ext
    q = _plan(C, name, 3, fwd=False)
    inp = dk.direct_inputs(name, 3, seed=5, device=DEV)
    wd, wsh = ics.desc(dc.JOB_WGRAD), dc.JOB_WGRAD
    wq = plans.wgrad_plan(wd)
    assert wq.cfg == 0
    wn = wq.nsplit * wsh[3] * 16 * wsh[2]
    wi = ck.wgrad_inputs(wsh, seed=9, device=DEV)
    wg_alone = ck.guarded(wn, device=DEV)
    C.wgrad(wi["G"], wi["X"], wd, wg_alone)
    for en in ("bias_relu", "mask_colsum"):
        ep = dc.DIRECT_EPILOGUES[en]
        alone = _launch_direct(C, q, inp, ep, fwd=False)
        jf, jw = C.Job(), C.Job()
        fused = _launch_direct(C, q, inp, ep, job=jf)
        wg_job = ck.guarded(wn, device=DEV)
        C.wgrad(wi["G"], wi["X"], wd, wg_job, job=jw)
        assert jf.kind > 0 and jw.kind > 0 and not jf.has_post
        bufs = [v for v in fused.values() if v is not None] + [wg_job]
        assert all(ck.untouched(b) for b in bufs)
        launched = C.launch_jobs([jf, jw])
        assert launched == dc.DIRECT_JOBS[name], f"{name}: kCombos"
        if launched:
            for k, v in fused.items():
                assert v is None or ck.same_bits(v, alone[k]), f"{name} {en}: {k} differs from its own launch"
            assert ck.same_bits(wg_job, wg_alone), f"{name} {en}: weight gradient differs from its own launch"
        else:
            assert all(ck.untouched(b) for b in bufs), f"{name} {en}: a refused job launch wrote to its outputs"


# --------------------------------------------------------- weight gradients ----
@pytest.mark.parametrize("name", list(dc.DWGRAD))
def test_direct_wgrad(name, native_ext, monkeypatch):
    C = native_ext
    cfg, H, Ci, CO, l2 = dc.DWGRAD[name]
    if l2:
        monkeypatch.setenv("MDT_DWGRAD_L2", "1")
    else:
        monkeypatch.delenv("MDT_DWGRAD_L2", raising=False)
    for N, exact in [(n, False) for n in dc.DWGRAD_N] + [(3, True)]:
        d = dc.desc(N, H, H, Ci, CO)
        q = plans.wgrad_plan(d)
        assert q.cfg == cfg and q.nsplit == N, q
        numel = CO * 16 * Ci
        inp = dk.dwgrad_inputs(name, N, seed=N, device=DEV, exact=exact)
        out = ck.guarded(N * numel, device=DEV)
        job = C.Job()
        C.wgrad(inp["G"], inp["X"], d, out, job=job)
        assert job.kind == 0 and ck.untouched(out), f"{name}: the direct weight gradient records no job"
        C.wgrad(inp["G"], inp["X"], d, out)
        assert ck.written(out, N * numel), f"{name} N={N}: unwritten row element or overrun guard"
        if exact:
            slabs, _ = ck.wgrad_ref(dk.dwgrad_shape(name, N), inp, (H // 2) ** 2 // 64)
            got = out[:N * numel].view(N, CO, 16 * Ci)
            assert all(dk.bits_equal(got[i], r) for i, (r, _) in enumerate(slabs)), f"{name}: exact rows differ"
        else:
            worst, total = dk.check_dwgrad(out, name, N, inp)
            _ok(f"{name} N={N} worst image row", worst)
            _ok(f"{name} N={N} row sum", total)


@pytest.mark.parametrize("x_f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("g", dc.THIN_WGRAD, ids=lambda g: f"N{g[0]}-{g[1]}x{g[2]}")
def test_thin_wgrad(g, x_f32, native_ext):
    C = native_ext
    N, H, W = g
    d = dc.desc(N, H, W, 1, 32)
    q = plans.wgrad_plan(d)
    assert q.cfg == plans.WG_THIN_MFMA and q.nsplit == N * (H // 2) // 4, q
    ns = q.nsplit
    inp = dk.thin_inputs(32, g, x_f32, seed=3, device=DEV)
    out = ck.guarded(ns * 512, device=DEV)
    C.wgrad(inp["G"], inp["x"], d, out)
    assert ck.written(out, ns * 512)
    worst, total = dk.check_thin_wgrad(out, inp["x"], inp["G"], x_f32)
    tag = f"thin_wgrad {g} {'f32' if x_f32 else 'bf16'}"
    _ok(tag + " worst row", worst)
    _ok(tag + " row sum", total)
    # exact data: every row bit for bit (f32 x needs all three bf16 terms)
    x, G, unit = dk.exact_thin_wgrad(x_f32, g, seed=4, device=DEV)
    assert not x_f32 or dk.terms_nonzero(x)
    out = ck.guarded(ns * 512, device=DEV)
    C.wgrad(G, x, d, out)
    slabs, _ = dk.thin_wgrad_refs(x, G, x_f32)
    got = out[:ns * 512].view(ns, 32, 16)
    Ga, ca = G.to(ck.F64).abs().reshape(-1, 32), ck.im2col(x.to(ck.F64).abs().unsqueeze(-1), 4, 2, 1)
    for i, (r, _) in enumerate(slabs):
        sl = slice(256 * i, 256 * i + 256)
        assert dk.exact_fits(1.02 * (Ga[sl].T @ ca[sl]), unit)
        assert dk.bits_equal(got[i], r), f"{tag}: exact row {i} differs"
    assert ck.written(out, ns * 512)


def test_thin_wgrad_job_form_is_bitwise(native_ext):
    """The MFMA thin weight gradient (bf16 X) next to a CO = 32 bf16 thin_conv job."""
    C = native_ext
    g = (3, 16, 128)
    d = dc.desc(*g, 1, 32)
    inp = dk.thin_inputs(32, g, False, seed=6, device=DEV)
    ns, M, nb = plans.wgrad_plan(d).nsplit, g[0] * 8 * 64, dc.thin_conv_blocks(g)

    def run(jobs):
        wg, y16, cs = ck.guarded(ns * 512, device=DEV), ck.guarded(M * 32, ck.BF, DEV), ck.guarded(nb * 32, device=DEV)
        C.wgrad(inp["G"], inp["x"], d, wg, **({"job": jobs[0]} if jobs else {}))
        C.thin_conv(inp["x"], inp["w"].flatten(), d, None, False, y16, inp["mask"].flatten(), cs,
                    **({"job": jobs[1]} if jobs else {}))
        return wg, y16, cs

    alone = run(None)
    jobs = (C.Job(), C.Job())
    fused = run(jobs)
    assert jobs[0].kind > 0 and jobs[1].kind > 0 and all(ck.untouched(b) for b in fused)
    assert C.launch_jobs(list(jobs)), "kCombos lists the MFMA thin weight gradient with ThinC32"
    for a, f, k in zip(alone, fused, ("wgrad", "y16", "colsum")):
        assert ck.same_bits(a, f), f"job form: {k} differs from its own launch"


# ---------------------------------------------------------------- thin_conv ----
def _thin_conv(C, CO, g, x, w, bias, relu, mask, colsum, **kw):
    M, nb = g[0] * (g[1] // 2) * (g[2] // 2), dc.thin_conv_blocks(g)
    y16 = ck.guarded(M * CO, ck.BF, DEV)
    cs = ck.guarded(nb * CO, device=DEV) if colsum else None
    C.thin_conv(x, w.flatten().contiguous(), dc.desc(*g, 1, CO), bias, relu, y16, mask, cs, **kw)
    assert ck.written(y16, M * CO) and (cs is None or ck.written(cs, nb * CO)), "unwritten output or overrun guard"
    return y16, cs


def _check_thin_conv(tag, CO, g, x, w, bias, relu, mask, y16, cs, exact_unit=None):
    M = g[0] * (g[1] // 2) * (g[2] // 2)
    acc, mag = dk.thin_conv_acc(x, w)
    ref, m = dk.thin_epilogue(acc, mag, bias, relu, mask)
    if exact_unit is not None:
        assert dk.exact_fits(1.02 * m, exact_unit)
        assert torch.equal(y16[:M * CO].view(M, CO), ref.to(ck.BF)), f"{tag}: y16 is not the rounded exact value"
    b = dk.thin_conv_bound(m, CO, g)
    _ok(tag + " y16", dk.y16_ratio(y16[:M * CO], ref, b))
    if cs is not None:
        cref, cb = dk.thin_colsum_ref(ref, b)
        got = cs[:cref.numel()].view(cref.shape)
        if exact_unit is not None:
            cmag, _ = dk.thin_colsum_ref(m, m)
            assert dk.exact_fits(1.02 * cmag, exact_unit)
            assert dk.bits_equal(got, cref), f"{tag}: column sums differ from the exact oracle"
        else:
            _ok(tag + " column sums", dk.ratio(got, cref, cb))


THIN_CONV = dc.THIN_CONV_VALU + dc.THIN_CONV_MFMA


@pytest.mark.parametrize("x_f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("CO,g", THIN_CONV, ids=[dc.gid(*c) for c in THIN_CONV])
def test_thin_conv(CO, g, x_f32, native_ext):
    C = native_ext
    assert C.thin_blocks(False, dc.desc(*g, 1, CO)) == dc.thin_conv_blocks(g)
    assert (plans.wgrad_plan(dc.desc(*g, 1, CO)).cfg == plans.WG_THIN_MFMA) == dc.thin_mfma_geom(CO, g)   # the body the host picks
    inp = dk.thin_inputs(CO, g, x_f32, seed=CO + g[1], device=DEV)
    for en, ep in dc.THIN_CONV_EPILOGUES.items():
        bias, mask = (inp["bias"] if ep["bias"] else None), (inp["mask"] if ep["mask"] else None)
        y16, cs = _thin_conv(C, CO, g, inp["x"], inp["w"], bias, ep["relu"], None if mask is None else mask.flatten(),
                             ep["colsum"])
        _check_thin_conv(f"thin_conv {dc.gid(CO, g)} {'f32' if x_f32 else 'bf16'} {en}", CO, g, inp["x"], inp["w"],
                         bias, ep["relu"], mask, y16, cs)


@pytest.mark.parametrize("kind,CO,g", [("ints", 16, (2, 28, 28)), ("ints", 32, (3, 10, 14)), ("ints", 64, (2, 28, 28)),
                                       ("ints", 32, (3, 16, 128)), ("x3", 32, (3, 16, 128)), ("w3", 32, (3, 16, 128)),
                                       ("w3", 32, (1, 8, 128))])
def test_thin_conv_exact(kind, CO, g, native_ext):
    """Exact data: the column sums (f32, stored unrounded) equal the oracle bit
    for bit. "x3" inputs and "w3" weights need all three bf16 terms of the MFMA
    body's hi/lo/lo2 split; a dropped term changes bits."""
    C = native_ext
    x, w, bias, unit = dk.exact_thin_conv(kind, CO, g, seed=2, device=DEV)
    assert kind != "x3" or dk.terms_nonzero(x)
    assert kind != "w3" or dk.terms_nonzero(w)
    mask = dk.thin_inputs(CO, g, True, seed=1, device=DEV)["mask"]
    for xx in ([x] if kind == "x3" else [x, x.to(ck.BF)]):      # {0..3} is exact in bf16: both input types
        y16, cs = _thin_conv(C, CO, g, xx, w, bias, False, mask.flatten(), True)
        _check_thin_conv(f"thin_conv exact {kind} {dc.gid(CO, g)} {xx.dtype}", CO, g, xx, w, bias, False, mask, y16, cs,
                         exact_unit=unit)


def _state(C, step=1):
    from tests.conv_small_checker import ADAM_SETS

    hp = ADAM_SETS["default"]
    st = C.TrialState(0)
    st.set_hparams(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], 1.0, hp["grad_scale"], 0,
                   hp["decoupled"], lr_warmup_steps=hp["lr_warmup_steps"], kl_anneal_steps=0)
    st.set_step(False, step)
    return st


@pytest.mark.parametrize("CO,g,with_hp", dc.THIN_CONV_GATHER, ids=[dc.gid(c, g) for c, g, _ in dc.THIN_CONV_GATHER])
def test_thin_conv_gather_is_bitwise(CO, g, with_hp, native_ext):
    """The gather form (first layer of a step: rows idx[cursor B + n] of the
    dataset) against the plain launch on the pre-gathered rows."""
    C = native_ext
    N, H, W = g
    rows, B, cursor, nbat = 11, N + 1, 2, 4
    gen = torch.Generator().manual_seed(N)
    X = torch.rand(rows, H * W, generator=gen).to(DEV)
    idx = torch.randint(0, rows, (nbat * B,), generator=gen, dtype=torch.int32).to(DEV)
    inp = dk.thin_inputs(CO, g, True, seed=8, device=DEV)
    pre = X[idx[cursor * B:cursor * B + N].long()].contiguous()
    y_ref, cs_ref = _thin_conv(C, CO, g, pre.view(N, H, W), inp["w"], inp["bias"], True, None, True)
    st = _state(C, step=5)
    st.set_cursor(False, cursor, nbat)
    xb = ck.guarded(N * H * W, device=DEV)
    y16, cs = _thin_conv(C, CO, g, X, inp["w"], inp["bias"], True, None, True, idx=idx, state=st.train_state,
                         hparams=st.hparams if with_hp else None, B=B, xb=xb)
    torch.cuda.synchronize()
    assert ck.same_bits(y16, y_ref) and ck.same_bits(cs, cs_ref)
    assert ck.written(xb, N * H * W) and torch.equal(xb[:N * H * W].view(N, -1), pre)
    rs = st.read_state(False)
    assert rs[0] == (6 if with_hp else 5) and rs[1] == cursor, rs


# --------------------------------------------------------------- thin_tconv ----
def _thin_tconv(C, CO, g, G, w, bias, names, tgt=None):
    N, H, W = g
    npix, nb = N * H * W, dc.thin_tconv_blocks(CO, g)
    out = {}
    for k in names:
        if k == "X":
            continue
        out[k] = ck.guarded(nb if k in ("part", "gpart") else npix, ck.BF if k == "dlog16" else torch.float32, DEV)
    kw = dict(out)
    if "X" in names:
        kw["X"] = tgt.flatten()
    C.thin_tconv(G, w.flatten().contiguous(), dc.desc(*g, 1, CO), bias, **kw)
    for k, v in out.items():
        assert ck.written(v, nb if k in ("part", "gpart") else npix), f"{k}: unwritten or overrun guard"
    return out


ALL_OUT = dc.THIN_TCONV_OUTPUTS[-1]
THIN_TCONV = dc.THIN_TCONV_VALU + dc.THIN_TCONV_PATCH


@pytest.mark.parametrize("CO,g", THIN_TCONV, ids=[dc.gid(*c) for c in THIN_TCONV])
def test_thin_tconv(CO, g, native_ext):
    C = native_ext
    N, H, W = g
    assert C.thin_blocks(True, dc.desc(*g, 1, CO)) == dc.thin_tconv_blocks(CO, g)
    inp = dk.thin_inputs(CO, g, True, seed=CO + H, device=DEV)
    out = _thin_tconv(C, CO, g, inp["G"], inp["tw"], inp["tbias"], ALL_OUT, inp["tgt"])
    t, mag = dk.thin_tconv_acc(inp["G"], inp["tw"], H, W, inp["tbias"])
    b_t = dk.thin_tconv_bound(mag, CO, g)
    tag = f"thin_tconv {dc.gid(CO, g)}"
    _ok(tag + " logits", dk.ratio(out["y32"][:t.numel()].view(t.shape), t, b_t))
    for k, r in dk.check_bce(out, t, b_t, inp["tgt"], dk.tconv_owners(CO, g, DEV)).items():
        _ok(f"{tag} {k}", r)


@pytest.mark.parametrize("CO,g", dc.THIN_TCONV_OPTIONAL_SHAPES, ids=[dc.gid(*c) for c in dc.THIN_TCONV_OPTIONAL_SHAPES])
def test_thin_tconv_optional_outputs_are_bitwise(CO, g, native_ext):
    C = native_ext
    inp = dk.thin_inputs(CO, g, True, seed=12, device=DEV)
    runs = [_thin_tconv(C, CO, g, inp["G"], inp["tw"], inp["tbias"], names, inp["tgt"])
            for names in dc.THIN_TCONV_OUTPUTS]
    full = runs[-1]
    for names, out in zip(dc.THIN_TCONV_OUTPUTS, runs):
        assert set(out) == set(names) - {"X"}
        for k, v in out.items():
            assert ck.same_bits(v, full[k]), f"{k} of {names} differs from the launch with every output"


@pytest.mark.parametrize("CO,g", dc.THIN_TCONV_OPTIONAL_SHAPES, ids=[dc.gid(*c) for c in dc.THIN_TCONV_OPTIONAL_SHAPES])
def test_thin_tconv_saturated_logits(CO, g, native_ext):
    """Logits beyond +-150: the 100 clamp, log1pf(expf(-|t|)) and expf(-t) = inf in the sigmoid."""
    C = native_ext
    N, H, W = g
    inp = dk.thin_inputs(CO, g, True, seed=13, device=DEV)
    tw = dk.saturate(inp["tw"], inp["G"], H, W, inp["tbias"])
    t, mag = dk.thin_tconv_acc(inp["G"], tw, H, W, inp["tbias"])
    assert float(t.min()) <= -150 and float(t.max()) >= 150
    x = inp["tgt"]
    assert bool((x == 0).any() and (x == 1).any() and ((x > 0) & (x < 1)).any())
    out = _thin_tconv(C, CO, g, inp["G"], tw, inp["tbias"], ALL_OUT, x)   # written() asserts everything finite
    b_t = dk.thin_tconv_bound(mag, CO, g)
    tag = f"thin_tconv saturated {dc.gid(CO, g)}"
    _ok(tag + " logits", dk.ratio(out["y32"][:t.numel()].view(t.shape), t, b_t))
    assert dk.saturated_recon_ok(out["recon"][:t.numel()], t), f"{tag}: recon not exactly 0 / 1"
    for k, r in dk.check_bce(out, t, b_t, x, dk.tconv_owners(CO, g, DEV)).items():
        _ok(f"{tag} {k}", r)


@pytest.mark.parametrize("kind,CO,g", [("ints", 16, (3, 10, 14)), ("ints", 32, (2, 28, 28)), ("ints", 64, (3, 10, 14)),
                                       ("ints", 32, (1, 128, 128)), ("w3", 32, (1, 128, 128))])
def test_thin_tconv_exact(kind, CO, g, native_ext):
    """Exact data: the f32 logits equal the oracle bit for bit; "w3" weights need
    all three bf16 terms of the MFMA body."""
    C = native_ext
    N, H, W = g
    G, w, bias, unit = dk.exact_thin_tconv(kind, CO, g, seed=3, device=DEV)
    assert kind != "w3" or dk.terms_nonzero(w)
    out = _thin_tconv(C, CO, g, G, w, bias, ("y32",))
    t, mag = dk.thin_tconv_acc(G, w, H, W, bias)
    assert dk.exact_fits(1.02 * mag, unit)
    assert dk.bits_equal(out["y32"][:t.numel()].view(t.shape), t), f"thin_tconv exact {kind} {dc.gid(CO, g)}"
