"""The checker of the importance-weighted pass's kernel tests (tests/iw_checker.py)
is not vacuous. For every oracle: (a) it agrees with an independent float64
route; (b) a plain f32 torch emulation of the kernel's formula and order passes
every bound at the GPU test's inputs (the worst error/bound ratio is printed);
(c) each mutated emulation (a bug the end-to-end tests could not see) fails it
on at least one element. Mutants live in these emulations only; no mutated
kernel exists."""
import math

import pytest
import torch
import torch.nn.functional as F

from multidisttorch_amd.models.iw import iw_prior_term, iw_reduce
from multidisttorch_amd.ops.philox import reparam_eps
from tests import iw_checker as ck

F32 = torch.float32
SEED = 11
NAN = float("nan")


def _eps(M, B, Z, k0, S, step, rows=None):
    """f32 eps [S, M, Z] of samples k0 .. k0 + S - 1; ``rows``: the row count the counter takes (B)."""
    rows = B if rows is None else rows
    e = torch.from_numpy(reparam_eps((k0 + S) * rows, Z, SEED, ck.IW_STREAM, step - 1)).view(k0 + S, rows, Z)
    return e[k0:, :M].contiguous()


# ------------------------------------------------------- f32 emulations ----
def emu_reparam(mulv, eps, mut=None):
    Z = mulv.shape[1] // 2
    mu, lv = mulv[:, :Z], mulv[:, Z:]
    z = mu + eps * torch.exp(0.5 * lv)
    zz = z.to(torch.bfloat16).float() if mut == "prior_from_bf16_z" else z
    term = -0.5 * zz * zz
    if mut != "no_eps2":
        term = term + 0.5 * eps * eps
    term = term + (-0.5 if mut == "lv_sign" else 0.5) * lv
    prior = torch.zeros(term.shape[:-1])
    for c in range(Z):   # one thread, latent order
        prior = prior + term[..., c]
    return z, prior


def emu_row_bce(t, x, mut=None):
    V, P = t.shape
    M = x.shape[0]
    rows = torch.arange(V) // (V // M) if mut == "row_v_div_S" else torch.arange(V) % M
    xv = x[rows]
    sp = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    cap = math.inf if mut == "no_clamp" else 100.0
    loss = xv * torch.clamp(sp - t, max=cap) + (1 - xv) * torch.clamp(sp, max=cap)
    n = -(-P // ck.LANES)
    loss = F.pad(loss, (0, n * ck.LANES - P)).view(V, n, ck.LANES)
    lane = torch.zeros(V, ck.LANES)
    for r in range(n):   # thread j: pixels j, j + 256, ...
        lane = lane + loss[:, r]
    w = ck.LANES
    while w > 1:         # the fixed tree
        w //= 2
        lane = lane[:, :w] + lane[:, w:2 * w]
    return lane[:, 0]


def emu_reduce(batches, B, K, S, mut=None):
    """iw_reduce_k over a pass: ``batches`` = [(prior [K, M], bce [K, M])] in f32.
    Returns (rows_nll, rows_ne) as the row buffers hold them (NaN = unwritten)."""
    st_m, st_s, st_l = torch.full((B,), -math.inf), torch.zeros(B), torch.zeros(B)
    out_n, out_e = [], []
    for prior, bce in batches:
        M = prior.shape[1]
        for k0, s in ck.chunks(K, S):
            first = k0 == 0 and mut != "no_reset"
            m = torch.full((M,), -math.inf) if first else st_m[:M].clone()
            ss = torch.zeros(M) if first else st_s[:M].clone()
            ls = torch.zeros(M) if first else st_l[:M].clone()
            for j in range(s - 1 if mut == "drop_last_of_chunk" else s):
                lw = prior[k0 + j] - bce[k0 + j]
                new = lw > m
                grow = ss + 1 if mut == "no_rescale" else ss * torch.exp(m - lw) + 1
                ss = torch.where(new, grow, ss + torch.exp(lw - m))
                m = torch.where(new, lw, m)
                ls = ls + lw
            st_m[:M], st_s[:M], st_l[:M] = m, ss, ls
        div = torch.tensor(float(s if mut == "log_S" else K), dtype=F32)
        nll = -(m + torch.log(ss) - torch.log(div))
        ne = -ls / div
        if mut == "skip_rows_256":
            nll[ck.LANES:], ne[ck.LANES:] = NAN, NAN
        out_n.append(nll)
        out_e.append(ne)
    return out_n, out_e


def _reduce_batches(case, pattern):
    M, B, K, S = case
    return [ck.reduce_inputs(pattern, K, Mb, seed=100 * b + M) for b, Mb in enumerate((B, M))]


def _reduce_ratio(case, pattern, mut=None):
    """Worst nll / neg_elbo ratio of the (mutated) emulation over both batches of a pass."""
    M, B, K, S = case
    batches = _reduce_batches(case, pattern)
    on, oe = emu_reduce(batches, B, K, S, mut)
    worst = 0.0
    for (prior, bce), nll, ne in zip(batches, on, oe):
        rn, re_, bn, be = ck.reduce_ref(*ck.lw_ref(prior, bce))
        worst = max(worst, ck.ratio(nll, rn, bn), ck.ratio(ne, re_, be))
    return worst


# ------------------------------------------------ (a) independent routes ----
@pytest.mark.parametrize("pattern", ck.PATTERNS)
def test_reduce_ref_is_logsumexp_and_mean(pattern):
    prior, bce = ck.reduce_inputs(pattern, 50, 7)
    lw, _ = ck.lw_ref(prior, bce)
    nll, ne, _, _ = ck.reduce_ref(lw)
    torch.testing.assert_close(nll, -(torch.logsumexp(lw, 0) - math.log(50)), rtol=1e-13, atol=0)
    a, e = iw_reduce(lw)
    torch.testing.assert_close(nll, a, rtol=1e-13, atol=0)
    torch.testing.assert_close(ne, e, rtol=1e-13, atol=0)
    if pattern == "equal":
        torch.testing.assert_close(nll, -lw[0], rtol=1e-13, atol=0)
    if pattern == "spread200":   # the others lie >= 100 nats under the maximum
        torch.testing.assert_close(nll, -lw.max(0).values + math.log(50), rtol=1e-15, atol=0)


def test_reparam_ref_is_the_models_prior_term():
    M, B, Z, k0, S = ck.REPARAM_CASES[1]
    mulv, eps = ck.reparam_mulv(M, Z).double(), _eps(M, B, Z, k0, S, 1).double()
    z, _, prior, _ = ck.reparam_ref(mulv, eps)
    q = torch.distributions.Normal(mulv[:, :Z], torch.exp(0.5 * mulv[:, Z:]))
    want = torch.distributions.Normal(0.0, 1.0).log_prob(z).sum(-1) - q.log_prob(z).sum(-1)   # log p(z) - log q(z|x)
    torch.testing.assert_close(prior, want, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(prior, iw_prior_term(z, eps, mulv[:, Z:]), rtol=1e-13, atol=1e-13)


def test_row_bce_ref_is_clamped_softplus():
    V, M, P = ck.ROW_BCE_CASES[4]
    t, x = ck.row_bce_inputs(V, M, P)
    ref, _ = ck.row_bce_ref(t, x, ck.conv_depth(P))
    t, xv = t.double(), x.double()[torch.arange(V) % M]
    sp = lambda a: torch.clamp(F.softplus(a, threshold=1e4), max=100.0)
    torch.testing.assert_close(ref, (xv * sp(-t) + (1 - xv) * sp(t)).sum(-1), rtol=1e-12, atol=0)


def test_totals_ratio_sees_one_row():
    rows = (540.0 + 10 * torch.rand(557, generator=ck.gen(1))).float()
    total = float(rows.double().sum())
    assert ck.totals_ratio(total, rows) == 0.0
    assert ck.totals_ratio(float(rows.double().flip(0).cumsum(0)[-1]), rows) <= 1   # another order
    assert ck.totals_ratio(total - float(rows[200]), rows) > 1e9                      # a dropped row
    assert ck.totals_ratio(total + float(rows[3]), rows) > 1e9                        # a doubled row
    assert ck.totals_ratio(float(rows.sum()), rows) > 1                               # an f32 sum


# ------------------------------------------------------- (b) + (c) ----
def test_eps_keys_on_the_trainers_batch_size():
    for M, B, Z, k0, S in ck.REPARAM_CASES:
        for step in ck.REPARAM_STEPS:
            assert ck.eps_ratio(_eps(M, B, Z, k0, S, step), B, Z, k0, SEED, step) == 0.0
            if M != B and k0 + S > 1:   # the counter taking M instead of B
                r = ck.eps_ratio(_eps(M, B, Z, k0, S, step, rows=M), B, Z, k0, SEED, step)
                print(f"MUTANT eps.counter_M M={M} B={B} ratio {r:.3g}")
                assert r > 1
            assert ck.eps_ratio(_eps(M, B, Z, k0, S, step + 1), B, Z, k0, SEED, step) > 1   # the batch index


REPARAM_MUTANTS = ("prior_from_bf16_z", "lv_sign", "no_eps2")


def test_reparam_emulation_passes_and_mutants_fail():
    worst = {"z": 0.0, "prior": 0.0}
    failed = {m: 0 for m in REPARAM_MUTANTS}
    for M, B, Z, k0, S in ck.REPARAM_CASES:
        mulv, eps = ck.reparam_mulv(M, Z), _eps(M, B, Z, k0, S, 1)
        z, bz, prior, bp = ck.reparam_ref(mulv, eps)
        gz, gp = emu_reparam(mulv, eps)
        worst["z"] = max(worst["z"], ck.ratio(gz, z, bz))
        worst["prior"] = max(worst["prior"], ck.ratio(gp, prior, bp))
        for mut in REPARAM_MUTANTS:
            failed[mut] += ck.ratio(emu_reparam(mulv, eps, mut)[1], prior, bp) > 1
    print("EMULATION reparam worst error/bound", worst)
    print("MUTANT reparam: cases failed of", len(ck.REPARAM_CASES), failed)
    assert worst["z"] <= 1 and worst["prior"] <= 1
    assert all(n == len(ck.REPARAM_CASES) for n in failed.values()), failed


def test_row_bce_emulation_passes_and_mutants_fail():
    worst = 0.0
    for V, M, P in ck.ROW_BCE_CASES:
        t, x = ck.row_bce_inputs(V, M, P)
        ref, bound = ck.row_bce_ref(t, x, ck.conv_depth(P))
        worst = max(worst, ck.ratio(emu_row_bce(t, x), ref, bound))
        if M > 1:
            assert len({tuple(r.tolist()) for r in x}) == M
            # pairing has power at every virtual row: the oracle with the image rows rolled by one fails
            rolled, _ = ck.row_bce_ref(t, x.roll(1, 0), ck.conv_depth(P))
            assert bool(((rolled - ref).abs() > bound).all()), (V, M, P)
        if V > M > 1:
            r = ck.ratio(emu_row_bce(t, x, "row_v_div_S"), ref, bound)
            print(f"MUTANT row_bce.row_v_div_S V={V} M={M} P={P} ratio {r:.3g}")
            assert r > 1
        if P >= 27:   # holds every planted logit
            r = ck.ratio(emu_row_bce(t, x, "no_clamp"), ref, bound)
            print(f"MUTANT row_bce.no_clamp V={V} M={M} P={P} ratio {r:.3g}")
            assert r > 1
    print(f"EMULATION row_bce worst error/bound {worst:.3g}")
    assert worst <= 1


def test_mlp_row_bce_emulation_passes_and_mutants_fail():
    """iw_dec_bce_k's oracle: logits from the stored h3 with their GEMM bound carried into the row sum."""
    g = ck.gen(3)
    S, M, H, D = 5, 37, 36, 100
    V = S * M
    h3 = torch.relu(torch.randn(V, H, generator=g))
    W4, b4 = 6.0 * torch.randn(D, H, generator=g), torch.randn(D, generator=g)
    x = torch.rand(M, D, generator=g)
    x[0::2] = (x[0::2] > 0.5).float()
    t, bt = ck.gemm_ref(h3, W4.t(), b4)
    assert float(t.abs().max()) > 100
    ref, bound = ck.row_bce_ref(t, x, ck.mlp_depth(D), bt)
    xv = x[torch.arange(V) % M]

    def emu(mut=None):
        tt = h3 @ W4.t() + b4
        sp = torch.clamp(tt, min=0) + torch.log1p(torch.exp(-tt.abs()))
        cap = math.inf if mut == "no_clamp" else 100.0
        xx = x[torch.arange(V) // S] if mut == "row_v_div_S" else xv
        return (xx * torch.clamp(sp - tt, max=cap) + (1 - xx) * torch.clamp(sp, max=cap)).sum(-1)

    r = ck.ratio(emu(), ref, bound)
    print(f"EMULATION mlp row_bce worst error/bound {r:.3g}")
    assert r <= 1
    for mut in ("no_clamp", "row_v_div_S"):
        rm = ck.ratio(emu(mut), ref, bound)
        print(f"MUTANT mlp_row_bce.{mut} ratio {rm:.3g}")
        assert rm > 1


@pytest.mark.parametrize("case", ck.REDUCE_CASES + [(7, 16, 500, 64)])
def test_reduce_emulation_passes(case):
    for pattern in ck.PATTERNS:
        r = _reduce_ratio(case, pattern)
        print(f"EMULATION reduce M,B,K,S={case} {pattern} worst error/bound {r:.3g}")
        assert r <= 1, (case, pattern, r)


# mutant -> the cases (indices into REDUCE_CASES) at which it must show
REDUCE_MUTANTS = {
    "no_rescale": (1, 2, 3, 4),          # K > 1
    "no_reset": (1, 2, 3, 4),            # the previous batch (or chunk) leaks in
    "log_S": (1, 2, 3),                  # the last chunk is shorter than K
    "drop_last_of_chunk": (1, 2, 3, 4),
    "skip_rows_256": (3, 4),             # M > 256
}


@pytest.mark.parametrize("mut", list(REDUCE_MUTANTS))
def test_reduce_mutants_fail(mut):
    for ci in REDUCE_MUTANTS[mut]:
        case = ck.REDUCE_CASES[ci]
        rs = {p: _reduce_ratio(case, p, mut) for p in ck.PATTERNS}
        print(f"MUTANT reduce.{mut} M,B,K,S={case}", " ".join(f"{p}={r:.3g}" for p, r in rs.items()))
        assert max(rs.values()) > 1, (mut, case)
    if mut == "no_rescale":   # seen by every pattern that climbs
        assert _reduce_ratio(ck.REDUCE_CASES[2], "ascending", mut) > 1
        assert _reduce_ratio(ck.REDUCE_CASES[2], "max_last", mut) > 1


@pytest.mark.parametrize("case", [c for c in ck.REDUCE_CASES if c[2] > 1])
def test_reduce_patterns_have_power(case):
    """A condition on the inputs, not a measurement: with any one sample removed
    (the divisor K kept), the oracle leaves the nll or the neg_elbo bound at every row."""
    M, B, K, S = case
    for pattern in ck.PATTERNS:
        if pattern == "spread200":
            continue
        for prior, bce in _reduce_batches(case, pattern):
            lw, b = ck.lw_ref(prior, bce)
            nll, ne, bn, be = ck.reduce_ref(lw, b)
            for j in range(K):
                keep = [k for k in range(K) if k != j]
                n2, e2, _, _ = ck.reduce_ref(lw[keep], b[keep], K=K)
                assert bool((((n2 - nll).abs() > bn) | ((e2 - ne).abs() > be)).all()), (case, pattern, j)
