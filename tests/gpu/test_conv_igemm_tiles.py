"""Every tile configuration of igemm_fwd_k (F0..F7, conv and parity mode, vector
and thin gathers), of wgrad_k (W0..W5, vector and thin, both store epilogues)
and the split-K combine against float64 oracles, element by element, under the
derived bound of tests/igemm_checker.py -- (K + 9) 2^-23 sum|a||w| and its
split-K, weight-gradient and column-sum forms -- plus bitwise identities (the
bf16 twin of an f32 output, the job form of a kernel against its stand-alone
launch) and poisoned guards behind every output.

Each case (tests/igemm_cases.py) reaches its configuration through the default
planner, as the trainer does; every test asks igemm_plan / wgrad_plan first and
asserts the configuration it is meant to hit before it launches anything.
References are float64 matmuls on the device. No tolerance here is measured.
"""
import pytest
import torch

from multidisttorch_amd.ops import conv_plans as plans
from tests import igemm_cases as cs
from tests import igemm_checker as ck

pytestmark = pytest.mark.gpu

DEV = "cuda"
FWD = cs.fwd_cases()
VEC = [c for c in FWD if not c[2]]
WG = cs.wgrad_cases()
EPILOGUES = {"bias_relu": dict(bias=True, relu=True), "mask_colsum": dict(mask=True)}


def _plan(C, mode, shape, split=False):
    q = plans.igemm_plan(mode, cs.desc(shape), split)
    return dict(cfg=q.cfg, BM=q.bm, BN=q.bn, classes=q.classes, M=q.m, Ncols=q.ncols, K=q.k, mtiles=q.mtiles,
                ntiles=q.ntiles, ktiles=q.ktiles, ksplit=q.ksplit, colsum_rows=q.colsum_rows)


def _wplan(C, shape):
    q = plans.wgrad_plan(cs.desc(shape))
    return dict(cfg=q.cfg, BM=q.bm, BN=q.bn, cotiles=q.cotiles, ktiles=q.ktiles, mtiles=q.mtiles, nsplit=q.nsplit,
                mps=q.mt_per_split)


def _launch_fwd(C, mode, shape, inp, q, ep, job=None):
    """One forward-type launch (or its recording into ``job``) with epilogue
    ``ep`` into fresh poisoned buffers: dict(y16, y32, colsum or None)."""
    n = q["classes"] * q["M"] * q["Ncols"]
    out = dict(y16=ck.guarded(n, ck.BF, DEV), y32=ck.guarded(n, device=DEV), colsum=None)
    mask = None
    if ep.get("mask"):
        mask = inp["mask"].flatten()
        out["colsum"] = ck.guarded(q["colsum_rows"] * q["Ncols"], device=DEV)
    C.igemm(mode, inp["A"], inp["B16"], cs.desc(shape), inp["bias"] if ep.get("bias") else None,
            bool(ep.get("relu")), out["y16"], out["y32"], mask, out["colsum"], job=job)
    return out


def _check_fwd(tag, mode, shape, inp, q, ep, out, acc, mag):
    n = q["classes"] * q["M"] * q["Ncols"]
    assert ck.written(out["y32"], n) and ck.written(out["y16"], n), f"{tag}: unwritten output or overrun guard"
    assert ck.twin_ok(out["y16"][:n], out["y32"][:n]), f"{tag}: y16 is not the bf16 rounding of y32"
    ref, m = ck.epilogue(acc, mag, inp, **ep)
    r = ck.check_fwd(out["y32"][:n], ref, m, q["K"])
    print(f"{tag}: error/bound {r:.4f}")
    assert r <= 1, f"{tag}: error/bound {r}"
    if out["colsum"] is not None:
        nc = q["colsum_rows"] * q["Ncols"]
        assert q["colsum_rows"] == q["classes"] * q["mtiles"]
        assert ck.written(out["colsum"], nc), f"{tag}: column sums unwritten or overrun"
        cref, cb = ck.colsum_ref(out["y32"][:n], mode, shape, q["BM"])
        rc = ck.ratio(out["colsum"][:nc].view(cref.shape), cref, cb)
        print(f"{tag}: column sums error/bound {rc:.4f}")
        assert rc <= 1, f"{tag}: column sums error/bound {rc}"


@pytest.mark.parametrize("name,mode,thin,cfg,shape", FWD, ids=[c[0] for c in FWD])
def test_igemm_tile(name, mode, thin, cfg, shape, native_ext):
    C = native_ext
    q = _plan(C, mode, shape)
    assert q["cfg"] == cfg and (q["BM"], q["BN"]) == cs.FWD_TILES[cfg] and q["ksplit"] == 1, q
    # by default only F6 and F7 can split (the other tiles need >= 512 blocks, split-K < 256): not forced here
    assert cfg in (6, 7) or _plan(C, mode, shape, True)["ksplit"] == 1
    for a_f32 in ((True, False) if thin else (False,)):
        inp = ck.fwd_inputs(mode, shape, a_f32=a_f32, seed=cfg, device=DEV)
        acc, mag = ck.fwd_acc(mode, shape, inp)
        # thin (first-layer) gathers: bias + ReLU for both A types; the others both epilogues
        for en in (("bias_relu",) if thin else EPILOGUES):
            ep = EPILOGUES[en]
            out = _launch_fwd(C, mode, shape, inp, q, ep)
            _check_fwd(f"{name} {'f32' if a_f32 else 'bf16'} A, {en}", mode, shape, inp, q, ep, out, acc, mag)


@pytest.mark.parametrize("cfg,ktiles,shape", cs.SPLITK, ids=[f"F{c}-kt{k}-CO{s[3]}" for c, k, s in cs.SPLITK])
def test_igemm_splitk_ragged(cfg, ktiles, shape, native_ext):
    """Raw slabs against the float64 partial sum over their own k-range, then
    the combined result (bias + ReLU in the combine pass)."""
    C = native_ext
    q = _plan(C, cs.CONV, shape, True)
    # blocks <= 3, so the planner splits down to one k-tile per slab; the last k-tile is partial
    assert q["cfg"] == cfg and q["ktiles"] == ktiles and q["ksplit"] == ktiles and q["K"] % 64, q
    M, N, ks = q["M"], q["Ncols"], q["ksplit"]
    inp = ck.fwd_inputs(cs.CONV, shape, seed=cfg, device=DEV)
    d = cs.desc(shape)
    ws, y32 = ck.guarded(ks * M * N, device=DEV), ck.guarded(M * N, device=DEV)
    C.igemm(cs.CONV, inp["A"], inp["B16"], d, inp["bias"], True, None, y32, ws=ws, combine=False)
    assert ck.written(ws, ks * M * N) and ck.untouched(y32)
    refs = ck.slab_refs(shape, inp, ktiles, 1)
    assert len(refs) == ks
    got = ws[:ks * M * N].view(ks, M, N)
    worst = max(ck.ratio(got[i], r, b) for i, (r, b) in enumerate(refs))
    print(f"split-K F{cfg} {shape}: worst slab error/bound {worst:.4f}")
    assert worst <= 1
    ws2, y16 = ck.guarded(ks * M * N, device=DEV), ck.guarded(M * N, ck.BF, DEV)
    C.igemm(cs.CONV, inp["A"], inp["B16"], d, inp["bias"], True, y16, y32, ws=ws2)
    assert ck.same_bits(ws, ws2)      # the slabs do not depend on the combine
    assert ck.written(y32, M * N) and ck.written(y16, M * N) and ck.twin_ok(y16[:M * N], y32[:M * N])
    ref, mag = ck.fwd_ref(cs.CONV, shape, inp, bias=True, relu=True)
    r = ck.check_fwd(y32[:M * N], ref, mag, q["K"], ks)
    print(f"split-K F{cfg} {shape}: combined error/bound {r:.4f}")
    assert r <= 1


@pytest.mark.parametrize("name,thin,x_f32,cfg,shape", WG, ids=[c[0] for c in WG])
def test_wgrad_tile(name, thin, x_f32, cfg, shape, native_ext):
    C = native_ext
    q = _wplan(C, shape)
    assert q["cfg"] == cfg and q["cfg"] < 100 and (q["BM"], q["BN"]) == cs.WG_TILES[cfg], q
    N, H, Ci, CO, k, s, p = shape
    numel = CO * k * k * Ci
    inp = ck.wgrad_inputs(shape, x_f32=x_f32, seed=cfg, device=DEV)
    out = ck.guarded(q["nsplit"] * numel, device=DEV)
    C.wgrad(inp["G"], inp["X"], cs.desc(shape), out)
    assert ck.written(out, q["nsplit"] * numel), f"{name}: unwritten slab element or overrun guard"
    worst, total = ck.check_wgrad(out, shape, inp, q["nsplit"], q["mps"])
    print(f"{name}: worst slab error/bound {worst:.4f}, slab sum {total:.4f} ({q['nsplit']} splits of {q['mps']})")
    assert worst <= 1 and total <= 1


@pytest.mark.parametrize("name,mode,thin,cfg,shape", VEC, ids=[c[0] for c in VEC])
def test_igemm_job_form_is_bitwise(name, mode, thin, cfg, shape, native_ext):
    """A kernel compared with itself, on purpose: the body of a forward GEMM and
    of the W0 weight gradient run as two jobs of one fused launch
    (conv_jobs.hip kCombos) must store exactly what their stand-alone launches
    store, guards included. Configurations without a job form launch nothing."""
    C = native_ext
    q = _plan(C, mode, shape)
    assert q["cfg"] == cfg, q
    wq = _wplan(C, cs.JOB_WGRAD)
    assert wq["cfg"] == 0, wq
    inp = ck.fwd_inputs(mode, shape, seed=cfg, device=DEV)
    wi = ck.wgrad_inputs(cs.JOB_WGRAD, seed=9, device=DEV)
    wd = cs.desc(cs.JOB_WGRAD)
    wn = wq["nsplit"] * cs.JOB_WGRAD[3] * 16 * cs.JOB_WGRAD[2]
    wg_alone = ck.guarded(wn, device=DEV)
    C.wgrad(wi["G"], wi["X"], wd, wg_alone)
    assert ck.written(wg_alone, wn)
    for en, ep in EPILOGUES.items():
        alone = _launch_fwd(C, mode, shape, inp, q, ep)
        jf, jw = C.Job(), C.Job()
        fused = _launch_fwd(C, mode, shape, inp, q, ep, job=jf)
        wg_job = ck.guarded(wn, device=DEV)
        C.wgrad(wi["G"], wi["X"], wd, wg_job, job=jw)
        assert jf.kind > 0 and jw.kind > 0 and not jf.has_post
        bufs = [v for v in fused.values() if v is not None] + [wg_job]
        assert all(ck.untouched(b) for b in bufs)        # recording launches nothing
        launched = C.launch_jobs([jf, jw])
        if cfg in cs.JOB_CFGS[mode]:
            assert launched, f"{name}: kCombos lists this configuration"
            for key, v in fused.items():
                assert v is None or ck.same_bits(v, alone[key]), f"{name} {en}: {key} differs from its own launch"
            assert ck.same_bits(wg_job, wg_alone), f"{name} {en}: weight gradient differs from its own launch"
        else:
            assert not launched
            assert all(ck.untouched(b) for b in bufs), f"{name} {en}: a refused job launch wrote to its outputs"
