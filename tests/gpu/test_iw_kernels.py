"""The importance-weighted pass's kernels against the float64 oracles and
derived bounds of tests/iw_checker.py.

Conv side and the shared reduce, each launched on its own through its binding
on planted inputs: iw_reparam (eps, z32, z16, prior), iw_row_bce, iw_reduce
(rows, pass totals, cursor, the rows_cap guard). Every output buffer is
poisoned (NaN; an out-of-band value for bf16) and longer than its logical
extent: inside, everything must be finite and within bound; outside, untouched.
Inputs come from fixed-seed CPU generators, the state from a fresh
``TrialState`` plus ``iw_state_new`` / ``iw_state_begin`` per launch.

MLP side (iw_sample_k, iw_dec_bce_k, iw_reduce_k inside ``evaluate_iw``), at
the shapes the pass really runs: the noise of sample k does not depend on K,
so passes whose K' are the chunk ends of the K-sample pass expose every chunk
in turn as "the last chunk" (``MlpVaeEngine.iw_act``), over batch 0 alone and
over batch 0 plus the tail. Each stage is checked against float64 from the
device's own inputs of that stage (eps, z and prior from mulv and eps, h3 from
z, the per-row BCE from h3), and every row of the pass against the reduce
oracle fed the float64 log-weights with those stages' bounds carried.

Each check prints ``RATIO <kernel>.<output> <error/bound>``."""
import math

import pytest
import torch

from tests import iw_checker as ck
from tests.conv_small_checker import BF16_FILL

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
SEED = 11
NAN = float("nan")
SEEN = {}


def _ok(name, r):
    SEEN[name] = max(SEEN.get(name, 0.0), r)
    print(f"RATIO {name} {r:.4g}")
    assert r <= 1, (name, r)


def _nan(n):
    return torch.full((n,), NAN, device=DEV)


def _fill16(n):
    return torch.full((n,), BF16_FILL, dtype=BF16, device=DEV)


def _tail_nan(t, n):
    t = t.cpu()
    assert bool(torch.isfinite(t[:n]).all()), "unwritten or non-finite element inside the logical extent"
    assert bool(torch.isnan(t[n:]).all()), "write past the logical extent"
    return t[:n]


def _padded(t, pad):
    """A CPU tensor, flattened, on the device with ``pad`` NaNs behind it (never to be read)."""
    return torch.cat([t.reshape(-1), torch.full((pad,), NAN)]).to(DEV)


def _hparams(C, seed=SEED):
    st = C.TrialState(0)
    st.set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, seed, False, lr_warmup_steps=0, kl_anneal_steps=0)
    return st


def _iw_state(C, nbatches, step=0):
    """A fresh pass state; ``step``: as the batch's first kernel leaves it (1 + the 0-based batch index)."""
    s = C.iw_state_new(0)
    C.iw_state_begin(s, nbatches)
    if step:
        s[:8].view(torch.int64).fill_(step)   # TrainState.step, the first field
    return s


def _read(C, s):
    return dict(zip(("nll", "neg_elbo", "step", "cursor"), C.iw_state_read(s)))


# --------------------------------------------------------------- iw_reparam ----
@pytest.mark.parametrize("step", ck.REPARAM_STEPS)
@pytest.mark.parametrize("M,B,Z,k0,S", ck.REPARAM_CASES)
def test_iw_reparam(M, B, Z, k0, S, step, native_ext):
    C = native_ext
    tst, ist = _hparams(C), _iw_state(C, 4, step)
    n = S * M * Z
    mulv = ck.reparam_mulv(M, Z, seed=M)
    z16, z32, eps, prior = _fill16(n + Z), _nan(n + Z), _nan(n + Z), _nan(S * M + 1)
    C.iw_reparam(_padded(mulv, 2 * Z), M, B, Z, k0, S, ist, tst.hparams, z16, z32, eps, prior)
    torch.cuda.synchronize()
    assert _read(C, ist)["step"] == step and _read(C, ist)["cursor"] == 0
    eps = _tail_nan(eps, n).view(S, M, Z)
    _ok("iw_reparam.eps", ck.eps_ratio(eps, B, Z, k0, SEED, step))
    z, bz, pr, bp = ck.reparam_ref(mulv, eps)
    got = _tail_nan(z32, n)
    _ok("iw_reparam.z32", ck.ratio(got.view(S, M, Z), z, bz))
    z16 = z16.cpu()
    assert bool((z16[n:].float() == BF16_FILL).all()), "z16: write past the logical extent"
    assert torch.equal(z16[:n], got.to(BF16)), "z16 is not the bf16 rounding of z32"
    _ok("iw_reparam.prior", ck.ratio(_tail_nan(prior, S * M).view(S, M), pr, bp))


def test_iw_reparam_refuses_out_of_domain(native_ext):
    """Each violation stops on the host: nothing is launched, the outputs keep their poison."""
    C = native_ext
    tst, ist = _hparams(C), _iw_state(C, 1, 1)
    n = 1 << 16
    z16, z32, eps, prior, mulv = _fill16(n), _nan(n), _nan(n), _nan(n), torch.zeros(n, device=DEV)
    bad = {"S*M > B": (5, 32, 8, 0, 7), "Z = 257": (1, 1, 257, 0, 1), "(k0+S)*B*Z > 2^32": (16, 16, 256, 1 << 20, 1),
           "M > B": (17, 16, 8, 0, 1), "Z = 0": (4, 16, 0, 0, 1), "k0 < 0": (4, 16, 8, -1, 1)}
    for name, (M, B, Z, k0, S) in bad.items():
        with pytest.raises(RuntimeError):
            C.iw_reparam(mulv, M, B, Z, k0, S, ist, tst.hparams, z16, z32, eps, prior)
            pytest.fail(f"accepted: {name}")
    torch.cuda.synchronize()
    assert bool((z16.float() == BF16_FILL).all())
    for t in (z32, eps, prior):
        assert bool(torch.isnan(t).all())
    assert _read(C, ist)["step"] == 1


# --------------------------------------------------------------- iw_row_bce ----
@pytest.mark.parametrize("V,M,P", ck.ROW_BCE_CASES)
def test_iw_row_bce(V, M, P, native_ext):
    C = native_ext
    t, x = ck.row_bce_inputs(V, M, P)
    ref, bound = ck.row_bce_ref(t, x, ck.conv_depth(P))
    if M > 1:   # the pairing has power at every virtual row (a condition on the inputs, checked before the launch)
        assert len({tuple(r.tolist()) for r in x}) == M
        rolled, _ = ck.row_bce_ref(t, x.roll(1, 0), ck.conv_depth(P))
        assert bool(((rolled - ref).abs() > bound).all())
    bce = _nan(V + 3)
    C.iw_row_bce(_padded(t, P), _padded(x, P), V, M, P, bce)
    torch.cuda.synchronize()
    _ok("iw_row_bce.bce", ck.ratio(_tail_nan(bce, V), ref, bound))


# ---------------------------------------------------------------- iw_reduce ----
def _reduce_pass(C, case, pattern, views=False):
    """A two-batch pass (B rows, then a tail of M). Returns the CPU row buffers
    [2B + 1] (``views``: the whole 2B allocation the B-element views sit in),
    the state after each batch and the oracles per batch."""
    M, B, K, S = case
    ist = _iw_state(C, 2)
    alloc = [_nan(2 * B + 1), _nan(2 * B + 1)]
    rows = [a[:B] for a in alloc] if views else alloc
    rowbuf = _nan(3 * B)
    states, refs = [], []
    for b, Mb in enumerate((B, M)):
        prior, bce = ck.reduce_inputs(pattern, K, Mb, seed=100 * b + M)
        rowbuf.fill_(NAN)   # a leak from the previous batch shows as NaN
        for k0, s in ck.chunks(K, S):
            C.iw_reduce(_padded(prior[k0:k0 + s], 1), _padded(bce[k0:k0 + s], 1), rowbuf, rows[0], rows[1], ist, Mb, B,
                        K, s, k0 == 0, k0 + s >= K)
        torch.cuda.synchronize()
        states.append(_read(C, ist))
        lw, b_lw = ck.lw_ref(prior, bce)
        refs.append((lw, ck.reduce_ref(lw, b_lw)))
    rb = rowbuf.cpu().view(3, B)
    assert bool(torch.isnan(rb[:, M:]).all()), "running state written past the batch's rows"
    return [a.cpu() for a in alloc], states, refs


@pytest.mark.parametrize("pattern", ck.PATTERNS)
@pytest.mark.parametrize("case", ck.REDUCE_CASES)
def test_iw_reduce(case, pattern, native_ext):
    C = native_ext
    M, B, K, S = case
    (rn, re_), states, refs = _reduce_pass(C, case, pattern)
    assert [s["cursor"] for s in states] == [1, 0], "the cursor must move 0 -> 1 -> 0"
    for b, Mb in enumerate((B, M)):   # rows at cursor * B + i
        lw, (nll, ne, bn, be) = refs[b]
        got_n, got_e = rn[b * B: b * B + Mb], re_[b * B: b * B + Mb]
        _ok(f"iw_reduce.row_nll[{pattern}]", ck.ratio(got_n, nll, bn))
        _ok(f"iw_reduce.row_neg_elbo[{pattern}]", ck.ratio(got_e, ne, be))
        if pattern == "equal":
            _ok("iw_reduce.row_nll[equal] = -lw", ck.ratio(got_n, -lw[0], bn))
        if pattern == "spread200":   # K e^-100 is below any f32 rounding
            _ok("iw_reduce.row_nll[spread200] = -max + log K", ck.ratio(got_n, -lw.max(0).values + math.log(K), bn))
    for r in (rn, re_):   # rows M .. B - 1 of the tail batch and the guard element
        assert bool(torch.isnan(r[B + M:]).all()), "write outside the batch's rows"
    n = B + M
    _ok("iw_reduce.total_nll", ck.totals_ratio(states[1]["nll"], rn[:n]))
    _ok("iw_reduce.total_neg_elbo", ck.totals_ratio(states[1]["neg_elbo"], re_[:n]))
    _ok("iw_reduce.total_nll (batch 0)", ck.totals_ratio(states[0]["nll"], rn[:B]))


def test_iw_reduce_rows_cap_guards_short_row_buffers(native_ext):
    """Row buffers of B elements (views into a poisoned 2B allocation): the
    second batch's rows are not written, its totals are still added."""
    C = native_ext
    case, pattern = ck.REDUCE_CASES[1], "spread10"
    M, B, K, S = case
    full, fstates, _ = _reduce_pass(C, case, pattern)
    part, pstates, _ = _reduce_pass(C, case, pattern, views=True)
    for f, p in zip(full, part):
        assert torch.equal(p[:B], f[:B])
        assert bool(torch.isnan(p[B:]).all()), "a row past the buffers' capacity was written"
    assert pstates == fstates, "the totals and the cursor do not depend on the row buffers' capacity"


# ----------------------------------------------------------------- MLP pass ----
def _gemm_blocks(A, Bm, bias, rows=2048):
    """mlp_checker.gemm_ref over row blocks of A (the float64 temporaries stay small)."""
    out = [ck.gemm_ref(A[i:i + rows], Bm, bias) for i in range(0, A.shape[0], rows)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


@pytest.mark.parametrize("name", list(ck.MLP_RUNS))
def test_mlp_pass_per_virtual_row(name, native_ext):
    from multidisttorch_amd.models.iw import iw_eps, mlp_encode
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    B, tail, D, H, Z, K, chunk, scaled = ck.MLP_RUNS[name]
    n = B + tail
    g = ck.gen(5)
    X = torch.rand(n, D, generator=g)
    X[0::2] = (X[0::2] > 0.5).float()   # every other image exact {0, 1}
    tr = MlpVaeTrainer(batch_size=B, D=D, H=H, Z=Z, device=torch.device(DEV, 0), backend="hip", seed=SEED,
                       use_graphs=False)
    v = tr.named_parameters()
    if scaled:
        with torch.no_grad():
            v["fc21.weight"].mul_(ck.MLP_SCALE)
            v["fc22.weight"].mul_(ck.MLP_SCALE)
            h = {k: t.detach().cpu() for k, t in v.items()}
            mu, lv = mlp_encode(h, X[:B])
            z = mu + torch.from_numpy(iw_eps(K, B, Z, SEED, 0)) * torch.exp(0.5 * lv)
            h3 = torch.relu(z.view(K * B, Z) @ h["fc3.weight"].t() + h["fc3.bias"])
            v["fc4.weight"].mul_(ck.LOGIT_PEAK / float((h3 @ h["fc4.weight"].t()).abs().max()))
    w = {k: t.detach().cpu().double() for k, t in v.items()}
    Xd, idx = X.to(DEV), torch.arange(n, dtype=torch.int32, device=DEV)
    S = ck.default_chunk(K, B, chunk)
    eng = tr.engine
    spread, clamped, first = 0.0, 0, None
    for b, Mb in enumerate((B, tail)):
        sub = idx[: b * B + Mb]
        x = X[b * B: b * B + Mb]
        lws, bounds = [], []
        for k0, s in ck.chunks(K, S):
            k1 = k0 + s
            r = tr.evaluate_iw(Xd, sub, k1, chunk_samples=chunk if k1 == K else S, return_rows=True)
            torch.cuda.synchronize()
            mulv = eng.act("mulv", Mb).cpu()
            eps, zd = eng.iw_act("eps", s, Mb).cpu(), eng.iw_act("z", s, Mb).cpu()
            prior, bce, h3 = eng.iw_act("prior", s, Mb).cpu(), eng.iw_act("bce", s, Mb).cpu(), eng.iw_act("h3", s, Mb).cpu()
            assert h3.shape == (s * Mb, H) and prior.shape == bce.shape == (s, Mb)
            _ok("iw_sample.eps", ck.eps_ratio(eps, B, Z, k0, SEED, b + 1))
            z, bz, pr, bp = ck.reparam_ref(mulv, eps)
            _ok("iw_sample.z", ck.ratio(zd, z, bz))
            _ok("iw_sample.prior", ck.ratio(prior, pr, bp))
            _ok("iw_sample.h3", ck.check_gemm(h3, zd.view(s * Mb, Z), w["fc3.weight"].t(), w["fc3.bias"], relu=True))
            t, bt = _gemm_blocks(h3, w["fc4.weight"].t(), w["fc4.bias"])
            br, bb, nc = ck.row_bce_ref(t, x, ck.mlp_depth(D), bt, want_clamped=True)
            clamped += nc
            _ok("iw_dec_bce.bce", ck.ratio(bce.view(-1), br, bb))
            lw, b_lw = ck.lw_ref(pr, br.view(s, Mb), bp, bb.view(s, Mb))
            lws.append(lw)
            bounds.append(b_lw)
        lw, b_lw = torch.cat(lws), torch.cat(bounds)
        spread = max(spread, float((lw.max(0).values - lw.min(0).values).max()))
        nll, ne, bn, be = ck.reduce_ref(lw, b_lw)
        assert r["rows"] == b * B + Mb and r["k"] == K
        rn, re_ = r["row_nll"].cpu(), r["row_neg_elbo"].cpu()
        _ok("iw_pass.row_nll", ck.ratio(rn[b * B:], nll, bn))
        _ok("iw_pass.row_neg_elbo", ck.ratio(re_[b * B:], ne, be))
        _ok("iw_pass.total_nll", ck.totals_ratio(r["nll"], rn))
        _ok("iw_pass.total_neg_elbo", ck.totals_ratio(r["neg_elbo"], re_))
        if b == 0:
            first = (rn, re_)
        else:   # batch 0 of the two-batch pass is the same function of (weights, data, seed, K)
            assert torch.equal(rn[:B], first[0]) and torch.equal(re_[:B], first[1])
    print(f"{name}: largest spread over k {spread:.3g} nats, clamped pixels {clamped}")
    if scaled:
        assert spread >= 5 and clamped > 0


def test_zz_report_largest_ratios():
    """Not a check of its own: prints the largest error/bound ratio each kernel output reached in this run."""
    for name in sorted(SEEN):
        print(f"MAXRATIO {name} {SEEN[name]:.4g}")
