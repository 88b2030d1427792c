"""The conv-VAE step's small kernels, each launched on its own against the
float64 oracles and derived bounds of tests/conv_small_checker.py: reparam,
reparam_bwd, combine_reparam(_bwd) in both forms, bce_logits, loss_finalize2,
colsum, adam_cast, grad_finalize's fused Adam and gather_rows, at the smallest
shapes that reach each of their paths.

Every output buffer is poisoned (NaN; an out-of-band value for bf16) and one
row / element longer than its logical extent: inside, everything must be
finite and within bound; the tail must be untouched. Inputs come from
fixed-seed CPU generators, the state from a fresh ``TrialState`` per launch.
Each check prints ``RATIO <kernel>.<output> <error/bound>``."""
import pytest
import torch

from tests import conv_small_checker as ck

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
SEEN = {}


def _ok(name, r):
    SEEN[name] = max(SEEN.get(name, 0.0), r)
    print(f"RATIO {name} {r:.4g}")
    assert r <= 1, (name, r)


def _nan(n):
    return torch.full((n,), float("nan"), device=DEV)


def _fill16(n):
    return torch.full((n,), ck.BF16_FILL, dtype=BF16, device=DEV)


def _tail_nan(t, n):
    t = t.cpu()
    assert bool(torch.isfinite(t[:n]).all()), "unwritten or non-finite element inside the logical extent"
    assert bool(torch.isnan(t[n:]).all()), "write past the logical extent"
    return t[:n]


def _tail16(t, n):
    t = t.cpu()
    assert bool((t[n:].float() == ck.BF16_FILL).all()), "write past the logical extent"
    return t[:n]


def _state(C, step=1, seed=0, kl_beta=1.0, kl_anneal=0, adam=None):
    """A fresh TrialState on device 0 at ``step`` (default hyper-parameters unless ``adam`` = an ADAM_SETS entry)."""
    hp = adam or ck.ADAM_SETS["default"]
    st = C.TrialState(0)
    st.set_hparams(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], kl_beta, hp["grad_scale"], seed,
                   hp["decoupled"], lr_warmup_steps=hp["lr_warmup_steps"], kl_anneal_steps=kl_anneal)
    st.set_step(False, step)
    return st


def _beta(C, anneal):
    """(TrialState, state argument, the KL weight the kernel must use): from
    HParams.kl_beta with no state, or from the state's kl_t under a KL-anneal
    schedule, whose value comes from the project's schedule oracle."""
    from multidisttorch_amd.hpo.schedule import Schedule

    if not anneal:
        st = _state(C, kl_beta=0.5)
        return st, None, 0.5
    st = _state(C, step=4, kl_beta=0.5, kl_anneal=10)
    beta = ck.f32(0.5 * Schedule(kl_anneal_steps=10).kl_factor(4))
    assert st.read_state(False)[6] == beta == ck.f32(0.2)
    return st, st.train_state, beta


def _host_eps(B, Z, seed=0, stream=0, step=0):
    from multidisttorch_amd.ops.philox import reparam_eps

    return torch.from_numpy(reparam_eps(B, Z, seed, stream, step))


# ------------------------------------------------------------------ reparam ----
# (B, Z, state step, seed, stream): one partial block; four blocks, the last partial, Z no power of two;
# the high counter word, seed_hi and the stream word all non-zero
REPARAM = [(5, 8, 1, 0, 0), (37, 24, 1, 0, 0), (5, 8, 2 ** 32 + 5, 2 ** 32 + 7, 3)]


def _check_reparam_outputs(tag, mulv, eps, z32, z16, kld, B, Z, owners):
    """z32 / z16 / kld_part against reparam_ref fed the kernel's own mulv and eps (CPU tensors, logical extents)."""
    z, k, _, bz, bk = ck.reparam_ref(mulv.view(B, 2 * Z), eps.view(B, Z))
    if z32 is not None:
        _ok(tag + ".z32", ck.ratio(z32.view(B, Z), z, bz))
        assert torch.equal(z16, z32.to(BF16)), tag + ": z16 is not the bf16 rounding of z32"
    else:
        _ok(tag + ".z16", ck.ratio(z16.view(B, Z), z, ck.bf16_bound(z, bz)))
    kref, kb = ck.block_sum_ref(k, bk, owners)
    _ok(tag + ".kld_part", ck.ratio(kld, kref, kb))


@pytest.mark.parametrize("with_z32", [True, False])
@pytest.mark.parametrize("B,Z,step,seed,stream", REPARAM)
def test_reparam(B, Z, step, seed, stream, with_z32, native_ext):
    C = native_ext
    st = _state(C, step=step, seed=seed)
    n, own = B * Z, ck.block_owners(B, Z)
    mulv = ck.reparam_inputs(B, Z)
    eps, z16, kld = _nan(n + Z), _fill16(n + Z), _nan(len(own) + 1)
    z32 = _nan(n + Z) if with_z32 else None
    C.reparam(mulv.to(DEV), eps, z16, z32, B, Z, st.train_state, st.hparams, stream, kld)
    torch.cuda.synchronize()
    eps = _tail_nan(eps, n)
    _ok("reparam.eps", ck.eps_ratio(eps, B, Z, seed, stream, step))
    _check_reparam_outputs("reparam", mulv, eps, _tail_nan(z32, n) if with_z32 else None, _tail16(z16, n),
                           _tail_nan(kld, len(own)), B, Z, own)


@pytest.mark.parametrize("anneal", [False, True])
@pytest.mark.parametrize("B,Z", [(5, 8), (37, 24)])
def test_reparam_bwd(B, Z, anneal, native_ext):
    C = native_ext
    st, state, beta = _beta(C, anneal)
    n = B * Z
    mulv, eps = ck.reparam_inputs(B, Z), _host_eps(B, Z)
    dz = torch.randn(B, Z, generator=ck.gen(5))
    ref, bound = ck.reparam_bwd_ref(dz, mulv, eps, beta)
    for with16 in (True, False):
        dmulv, d16 = _nan(2 * n + 2 * Z), _fill16(2 * n + 2 * Z)
        C.reparam_bwd(dz.to(DEV), mulv.to(DEV), eps.to(DEV), dmulv, d16 if with16 else None, B, Z, st.hparams,
                      state=state)
        torch.cuda.synchronize()
        got = _tail_nan(dmulv, 2 * n)
        _ok("reparam_bwd.dmulv", ck.ratio(got.view(B, 2 * Z), ref, bound))
        if with16:
            assert torch.equal(_tail16(d16, 2 * n), got.to(BF16)), "dmulv16 is not the bf16 rounding of dmulv"
        else:
            _tail16(d16, 0)   # not passed: untouched


# ----------------------------------------------------- split-K combines ----
def _grid(Z, fwd):
    return ck.row_ks(Z, fwd) if Z in ck.ROW_Z else list(ck.ELEM_KS)


@pytest.mark.parametrize("Z", ck.ROW_Z + ck.ELEM_Z)
def test_combine_reparam(Z, native_ext):
    C = native_ext
    B, stream, n = 3, 2, 3 * Z
    # the stand-alone kernel's noise at the same (state, stream): the counter is the same, so are the bits
    st = _state(C)
    eps0 = _nan(n)
    C.reparam(torch.zeros(B, 2 * Z, device=DEV), eps0, _fill16(n), None, B, Z, st.train_state, st.hparams, stream,
              _nan(n))
    eps0 = eps0.cpu()
    _ok("reparam.eps", ck.eps_ratio(eps0, B, Z, 0, stream, 1))
    grid = _grid(Z, True)
    for ks in grid:
        slab, bias = ck.slab_inputs(ks, B, Z, True, seed=ks)
        own = ck.block_owners(B, Z, ks)
        assert C.combine_reparam_blocks(ks, B, Z) == len(own)
        for with_bias, with_z32 in ((False, True), (True, True), (True, False)):
            if not with_z32 and ks != grid[-1]:
                continue
            st = _state(C)
            mulv, eps, z16, kld = _nan(2 * n + 2 * Z), _nan(n + Z), _fill16(n + Z), _nan(len(own) + 1)
            z32 = _nan(n + Z) if with_z32 else None
            C.combine_reparam(slab.to(DEV), ks, bias.to(DEV) if with_bias else None, mulv, eps, z16, z32, B, Z,
                              st.train_state, st.hparams, stream, kld)
            torch.cuda.synchronize()
            mulv = _tail_nan(mulv, 2 * n)
            _ok("combine_reparam.mulv", ck.ratio(mulv.view(B, 2 * Z), *ck.slab_sum_ref(slab[:ks],
                                                                                      bias if with_bias else None)))
            eps = _tail_nan(eps, n)
            assert torch.equal(eps, eps0), f"Z={Z} ks={ks}: noise differs from the stand-alone reparam's"
            _check_reparam_outputs("combine_reparam", mulv, eps, _tail_nan(z32, n) if with_z32 else None,
                                   _tail16(z16, n), _tail_nan(kld, len(own)), B, Z, own)


@pytest.mark.parametrize("anneal", [False, True])
@pytest.mark.parametrize("Z", ck.ROW_Z + ck.ELEM_Z)
def test_combine_reparam_bwd(Z, anneal, native_ext):
    C = native_ext
    B, n = 3, 3 * Z
    mulv, eps = ck.reparam_inputs(B, Z), _host_eps(B, Z)
    for ks in _grid(Z, False):
        slab, _ = ck.slab_inputs(ks, B, Z, False, seed=ks)
        st, state, beta = _beta(C, anneal)
        outs, dz = [], None
        for with_dz in (True, False):
            dmulv, d16 = _nan(2 * n + 2 * Z), _fill16(2 * n + 2 * Z)
            dzb = _nan(n + Z) if with_dz else None
            C.combine_reparam_bwd(slab.to(DEV), ks, mulv.to(DEV), eps.to(DEV), dmulv, d16, dzb, B, Z, st.hparams,
                                  state=state)
            torch.cuda.synchronize()
            outs.append((_tail_nan(dmulv, 2 * n), _tail16(d16, 2 * n)))
            if with_dz:
                dz = _tail_nan(dzb, n).view(B, Z)
        got, got16 = outs[0]
        _ok("combine_reparam_bwd.dz", ck.ratio(dz, *ck.slab_sum_ref(slab[:ks])))
        # dmulv is formed from the register that dz was stored from: no slab bound between them
        _ok("combine_reparam_bwd.dmulv", ck.ratio(got.view(B, 2 * Z), *ck.reparam_bwd_ref(dz, mulv, eps, beta)))
        assert torch.equal(got16, got.to(BF16)), f"Z={Z} ks={ks}: dmulv16 is not the bf16 rounding of dmulv"
        assert torch.equal(outs[1][0], got) and torch.equal(outs[1][1], got16), "dz=None changed the result"


# --------------------------------------------------------------- bce_logits ----
@pytest.mark.parametrize("use_rows", [False, True])
@pytest.mark.parametrize("B,P", [(3, 100), (2, 784)])
def test_bce_logits(B, P, use_rows, native_ext):
    C = native_ext
    t, x = ck.bce_inputs(B, P)
    n = B * P
    own = ck.block_owners(1, n)   # 256 consecutive elements per block
    if use_rows:   # an unsorted index with one repeated row into a larger X
        rows = [B + 1] + list(range(B - 2, 0, -1)) + [B + 1]
        X = torch.rand(B + 3, P, generator=ck.gen(9))
        X[B + 1] = x[0]
        X[B + 1, P - 20:] = x[B - 1, P - 20:]
        x = X[rows]
        rows_d = torch.tensor(rows, dtype=torch.int32, device=DEV)
    else:
        X, rows_d = x, None
    r = ck.bce_ref(t, x)
    assert int((r["loss"] == 100.0).sum()) == 4   # the clamp bites at the four +-120 logits
    pref, pb = ck.block_sum_ref(r["loss"], r["b_loss"], own)
    gref, gb = ck.block_sum_ref(r["g"], r["b_g"], own)
    for skip in (None, "dlog16", "recon", "gpart"):
        dlog, recon, part, gpart = _fill16(n + P), _nan(n + P), _nan(len(own) + 1), _nan(len(own) + 1)
        C.bce_logits(t.to(DEV), X.to(DEV), rows_d, B, P, None if skip == "dlog16" else dlog,
                     None if skip == "recon" else recon, part, None if skip == "gpart" else gpart)
        torch.cuda.synchronize()
        _ok("bce_logits.part", ck.ratio(_tail_nan(part, len(own)), pref, pb))
        if skip != "gpart":
            _ok("bce_logits.gpart", ck.ratio(_tail_nan(gpart, len(own)), gref, gb))
        if skip != "recon":
            _ok("bce_logits.recon", ck.ratio(_tail_nan(recon, n).view(B, P), r["p"], r["b_p"]))
        if skip != "dlog16":
            d = _tail16(dlog, n).view(B, P)
            _ok("bce_logits.dlog16", ck.ratio(d, r["g"], ck.bf16_bound(r["g"], r["b_g"])))
        else:
            _tail16(dlog, 0)


# ----------------------------------------------------------- loss_finalize2 ----
def _read(st):
    return dict(zip(("step", "cursor", "nbatches", "epoch_loss", "epoch_count", "lr", "kl"), st.read_state(False)))


def _partials(nb, nk, seed):
    """Small-integer partials (every sum exact in f32) followed by a NaN the kernel must not read."""
    g = ck.gen(seed)
    mk = lambda n: torch.cat([torch.randint(0, 9, (n,), generator=g).float(), torch.tensor([float("nan")])])
    return mk(nb), mk(nk)


@pytest.mark.parametrize("nb,nk", [(1, 1), (255, 257), (256, 256), (1000, 3)])
def test_loss_finalize2(nb, nk, native_ext):
    C = native_ext
    st = _state(C, step=7)
    st.set_cursor(False, 2, 4)
    total = 0.0
    for call in range(2):
        bce, kld = _partials(nb, nk, 10 * call + nb)
        C.loss_finalize2(bce.to(DEV), nb, kld.to(DEV), nk, st.train_state, st.hparams, True)
        torch.cuda.synchronize()
        loss = float(bce[:nb].sum() + kld[:nk].sum())   # kl_t = 1
        total += loss
        rs, hist = _read(st), st.loss_history(False)
        assert float(hist[6]) == loss and not hist[:6].any() and not hist[7:].any()   # slot (step - 1) % kLossHist
        assert (rs["step"], rs["epoch_loss"], rs["epoch_count"]) == (7, total, call + 1)
        assert rs["cursor"] == (3, 0)[call]   # advances, then wraps at nbatches = 4
    bce, kld = _partials(nb, nk, 99)
    C.loss_finalize2(bce.to(DEV), nb, kld.to(DEV), nk, st.train_state, st.hparams, False)
    assert _read(st)["cursor"] == 0 and _read(st)["epoch_count"] == 3   # advance_cursor = False
    st.set_cursor(False, 5, 0)
    for want_cursor in (6, 7):   # nbatches = 0: never wraps
        C.loss_finalize2(bce.to(DEV), nb, kld.to(DEV), nk, st.train_state, st.hparams, True)
        assert _read(st)["cursor"] == want_cursor


def test_loss_finalize2_advances_the_step(native_ext):
    from multidisttorch_amd.hpo.schedule import Schedule

    C = native_ext
    H, nb, nk = C.kLossHist, 255, 257
    sch = Schedule(kl_anneal_steps=10)
    st = _state(C, step=4, kl_beta=0.5, kl_anneal=10)
    for start in (4, H):   # -> step 5 (slot 4, KL weight 0.25) and H + 1 (the ring wraps to slot 0, weight 0.5)
        st.set_step(False, start)
        st.reset_loss(False)
        bce, kld = _partials(nb, nk, start)
        C.loss_finalize2(bce.to(DEV), nb, kld.to(DEV), nk, st.train_state, st.hparams, False, advance_step=True)
        torch.cuda.synchronize()
        rs, hist = _read(st), st.loss_history(False)
        kl = ck.f32(0.5 * sch.kl_factor(start + 1))
        assert kl in (0.25, 0.5)   # dyadic, so the weighted sum below is exact whether or not it is contracted
        loss = float(bce[:nb].sum()) + kl * float(kld[:nk].sum())
        assert rs["step"] == start + 1 and rs["kl"] == kl and rs["lr"] == 1e-3
        assert float(hist[start % H]) == loss and rs["epoch_loss"] == loss and rs["epoch_count"] == 1
        if start == 4:
            assert not hist[:4].any() and not hist[5:].any()


# ------------------------------------------------------------------- colsum ----
# a ragged last row group; one live thread; two column blocks (N / 8 > 256); rows_per > M
@pytest.mark.parametrize("M,N,rows_per", [(37, 64, 16), (5, 8, 8), (3, 2056, 4), (9, 16, 64)])
def test_colsum(M, N, rows_per, native_ext):
    C = native_ext
    G = torch.randint(-8, 9, (M + 1, N), generator=ck.gen(M)).float()
    G[M] = float("nan")   # a row the kernel must not read
    gy = -(-M // rows_per)
    slab = _nan(gy * N + N)
    C.colsum(G.to(BF16).to(DEV), M, N, rows_per, slab)
    torch.cuda.synchronize()
    want = torch.stack([G[y * rows_per:min(M, (y + 1) * rows_per)].sum(0) for y in range(gy)])
    assert torch.equal(_tail_nan(slab, gy * N).view(gy, N), want)


def test_multi_job_table_holds_eight_jobs(native_ext):
    """jobs_multi_k reads eight job starts (kMaxMultiJobs): packing refuses a
    ninth job, and a full table's grid is the sum of its jobs' workgroups."""
    C = native_ext
    G = torch.zeros(8 * 8, dtype=BF16, device=DEV)
    slabs = [torch.zeros(8, device=DEV) for _ in range(9)]
    jobs = [C.Job() for _ in range(9)]
    for j, slab in zip(jobs, slabs):
        C.colsum(G, 8, 8, 8, slab, job=j)   # the smallest shape: one workgroup
    with pytest.raises(RuntimeError):
        C.pack_jobs_multi(jobs)
    _, grid = C.pack_jobs_multi(jobs[:8])
    assert grid == sum(j.nblk for j in jobs[:8]) > 0


# ---------------------------------------------------------------- adam_cast ----
def _adam_bufs(total, seed=0):
    """P, G, m, v, w16 as logical views of buffers 4 elements longer (the guard tail), and the buffers."""
    p, g, m, v = ck.adam_inputs(total, seed)
    pad = lambda t: torch.cat([t, torch.full((4,), float("nan"))]).to(DEV)
    full = [pad(p), pad(g), pad(m), pad(v), _fill16(total + 4)]
    return (p, g, m, v), [t.narrow(0, 0, total) for t in full], full


def _check_adam(tag, host, full, total, c):
    p, g, m, v = host
    rp, rm, rv, bp, bm, bv = ck.adam_ref(p, g, m, v, c)
    P = _tail_nan(full[0], total)
    _ok(tag + ".P", ck.ratio(P, rp, bp))
    _ok(tag + ".m", ck.ratio(_tail_nan(full[2], total), rm, bm))
    _ok(tag + ".v", ck.ratio(_tail_nan(full[3], total), rv, bv))
    assert torch.equal(_tail16(full[4], total), P.to(BF16)), tag + ": w16 is not the bf16 rounding of P"
    assert torch.equal(_tail_nan(full[1], total), g)


# one float4; one block + one float4; the grid-stride loop past the 1024-block cap
@pytest.mark.parametrize("total", [4, 1028, 1024 * 256 * 4 + 8])
def test_adam_cast(total, native_ext):
    C = native_ext
    segs = torch.zeros(64, dtype=torch.uint8, device=DEV)
    host, view, full = _adam_bufs(total)
    st = _state(C)
    C.adam_cast(*view, segs, 0, st.train_state, st.hparams, False)
    torch.cuda.synchronize()
    for i in range(4):   # cast only: P, G, m, v untouched bitwise
        assert torch.equal(_tail_nan(full[i], total), host[i])
    assert torch.equal(_tail16(full[4], total), host[0].to(BF16))
    for name, hp in ck.ADAM_SETS.items():
        for step in (1, 1000):
            host, view, full = _adam_bufs(total, seed=step)
            assert total == 4 or int(((host[1] * hp["grad_scale"]) ** 2 > 77).sum()) > 50
            st = _state(C, step=step, adam=hp)
            assert st.read_state(False)[5] == ck.adam_consts(hp, step)["lr"]
            C.adam_cast(*view, segs, 0, st.train_state, st.hparams, True)
            torch.cuda.synchronize()
            _check_adam("adam_cast", host, full, total, ck.adam_consts(hp, step))


@pytest.mark.parametrize("cnt", [256, 1024])
@pytest.mark.parametrize("name", list(ck.ADAM_SETS))
def test_grad_finalize_fused_adam(name, cnt, native_ext):
    """grad_finalize(do_adam=True) against the oracle fed the gradient the same
    kernel finalizes with do_adam=False (scalar units and 4-element units)."""
    C = native_ext
    hp, step, numel, ns = ck.ADAM_SETS[name], 1000, 5000 + 2, 3
    slab = (3.0 * torch.randn(ns, numel, generator=ck.gen(3))).to(DEV)
    slab[:, ::5] *= 10.0
    segs = C.make_grad_segs([[0, numel, slab.data_ptr(), ns, 0, 0, 0, 0, -1]], 0)
    units = [[0, s, min(cnt, numel - s)] for s in range(0, numel, cnt)]
    U = C.make_grad_units(units, 0)
    st = _state(C, step=step, adam=hp)
    p, _, m, v = ck.adam_inputs(numel, seed=4)
    G = _nan(numel)
    P, M, V, w16 = p.to(DEV), m.to(DEV), v.to(DEV), _fill16(numel)
    C.grad_finalize(P, G, M, V, w16, segs, U, len(units), st.train_state, st.hparams, False)
    torch.cuda.synchronize()
    g = G.cpu()
    _ok("grad_finalize.G", ck.ratio(g, *ck.slab_sum_ref(slab.cpu())))
    assert torch.equal(P.cpu(), p) and torch.equal(w16.cpu().float(), torch.full((numel,), ck.BF16_FILL))
    full = [torch.cat([t, torch.full((4,), float("nan"))]).to(DEV) for t in (p, g, m, v)] + [_fill16(numel + 4)]
    view = [t.narrow(0, 0, numel) for t in full]
    G2 = _nan(numel)   # the fused path consumes the gradient in registers: G stays untouched
    C.grad_finalize(view[0], G2, view[2], view[3], view[4], segs, U, len(units), st.train_state, st.hparams, True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(G2).all())
    _check_adam("grad_finalize", (p, g, m, v), full, numel, ck.adam_consts(hp, step))


# -------------------------------------------------------------- gather_rows ----
# cursor 2 of 4 with a partial batch; 17 * 16384 float4s: past the 1024-block cap
@pytest.mark.parametrize("B,M,P,cursor,nb,rows", [(8, 5, 100, 2, 4, 40), (17, 17, 65536, 0, 1, 20)])
def test_gather_rows(B, M, P, cursor, nb, rows, native_ext):
    C = native_ext
    g = ck.gen(B)
    X = torch.rand(rows, P, generator=g)
    idx = torch.randint(0, rows, (nb * B,), generator=g, dtype=torch.int32)
    st = _state(C)
    st.set_cursor(False, cursor, nb)
    xb = _nan((M + 1) * P)
    C.gather_rows(X.to(DEV), idx.to(DEV), st.train_state, B, M, xb)
    torch.cuda.synchronize()
    assert torch.equal(_tail_nan(xb, M * P).view(M, P), X[idx[cursor * B:cursor * B + M].long()])


# --------------------------------------------------------- argument checks ----
def test_out_of_domain_arguments_raise(native_ext):
    """One violation of each condition the bindings check: the call must stop
    on the host (RuntimeError) and launch nothing."""
    C = native_ext
    st = _state(C)
    S, H = st.train_state, st.hparams
    f = lambda *s: torch.zeros(*s, device=DEV)
    h = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    B, Z, P, ks = 3, 8, 100, 2
    n = B * Z
    bad = {
        # reparam(mulv, eps, z16, z32, B, Z, state, hparams, stream, kld_part)
        "reparam: B = 0": lambda: C.reparam(f(2 * n), f(n), h(n), None, 0, Z, S, H, 0, f(1)),
        "reparam: Z = 0": lambda: C.reparam(f(2 * n), f(n), h(n), None, B, 0, S, H, 0, f(1)),
        "reparam: mulv short": lambda: C.reparam(f(2 * n - 1), f(n), h(n), None, B, Z, S, H, 0, f(1)),
        "reparam: eps bf16": lambda: C.reparam(f(2 * n), h(n), h(n), None, B, Z, S, H, 0, f(1)),
        "reparam: z16 f32": lambda: C.reparam(f(2 * n), f(n), f(n), None, B, Z, S, H, 0, f(1)),
        "reparam: mulv on the host": lambda: C.reparam(f(2 * n).cpu(), f(n), h(n), None, B, Z, S, H, 0, f(1)),
        "reparam: mulv strided": lambda: C.reparam(f(B, 4 * Z)[:, :2 * Z], f(n), h(n), None, B, Z, S, H, 0, f(1)),
        "reparam: kld_part short": lambda: C.reparam(f(600), f(300), h(300), None, 1, 300, S, H, 0, f(1)),
        "reparam: state short": lambda: C.reparam(f(2 * n), f(n), h(n), None, B, Z, S[:64], H, 0, f(1)),
        "reparam: z32 short": lambda: C.reparam(f(2 * n), f(n), h(n), f(n - 1), B, Z, S, H, 0, f(1)),
        # reparam_bwd(dz, mulv, eps, dmulv, dmulv16, B, Z, hparams, state)
        "reparam_bwd: dz short": lambda: C.reparam_bwd(f(n - 1), f(2 * n), f(n), f(2 * n), None, B, Z, H),
        "reparam_bwd: dmulv16 f32": lambda: C.reparam_bwd(f(n), f(2 * n), f(n), f(2 * n), f(2 * n), B, Z, H),
        "reparam_bwd: eps short": lambda: C.reparam_bwd(f(n), f(2 * n), f(n - 1), f(2 * n), None, B, Z, H),
        "reparam_bwd: Z = 0": lambda: C.reparam_bwd(f(n), f(2 * n), f(n), f(2 * n), None, B, 0, H),
        # bce_logits(logits, X, rows, B, P, dlog16, recon, part, gpart)
        "bce_logits: part short": lambda: C.bce_logits(f(B * P), f(B * P), None, B, P, None, None, f(1), None),
        "bce_logits: gpart short": lambda: C.bce_logits(f(B * P), f(B * P), None, B, P, None, None, f(2), f(1)),
        "bce_logits: X short": lambda: C.bce_logits(f(B * P), f(B * P - 1), None, B, P, None, None, f(2), None),
        "bce_logits: rows int64": lambda: C.bce_logits(f(B * P), f(B * P), torch.zeros(B, dtype=torch.int64,
                                                                                     device=DEV), B, P, None, None,
                                                       f(2), None),
        "bce_logits: rows short": lambda: C.bce_logits(f(B * P), f(B * P), i32(B - 1), B, P, None, None, f(2), None),
        "bce_logits: dlog16 f32": lambda: C.bce_logits(f(B * P), f(B * P), None, B, P, f(B * P), None, f(2), None),
        "bce_logits: P = 0": lambda: C.bce_logits(f(B * P), f(B * P), None, B, 0, None, None, f(2), None),
        # gather_rows(X, idx, state, B, M, xb)
        "gather_rows: P % 4": lambda: C.gather_rows(f(10, 6), i32(8), S, 8, 5, f(5 * 6)),
        "gather_rows: xb short": lambda: C.gather_rows(f(10, 8), i32(8), S, 8, 5, f(5 * 8 - 1)),
        "gather_rows: M > B": lambda: C.gather_rows(f(10, 8), i32(8), S, 4, 5, f(5 * 8)),
        "gather_rows: idx short": lambda: C.gather_rows(f(10, 8), i32(7), S, 8, 5, f(5 * 8)),
        "gather_rows: X 1-D": lambda: C.gather_rows(f(80), i32(8), S, 8, 5, f(5 * 8)),
        # colsum(G16, M, N, rows_per, slab, job), both forms
        "colsum: N % 8": lambda: C.colsum(h(5 * 12), 5, 12, 8, f(12)),
        "colsum: rows_per = 0": lambda: C.colsum(h(5 * 8), 5, 8, 0, f(8)),
        "colsum job: N % 8": lambda: C.colsum(h(5 * 12), 5, 12, 8, f(12), job=C.Job()),
        "colsum job: rows_per = 0": lambda: C.colsum(h(5 * 8), 5, 8, 0, f(8), job=C.Job()),
        "colsum: slab short": lambda: C.colsum(h(5 * 8), 5, 8, 2, f(2 * 8)),
        # combine_reparam(ws, ks, bias, mulv, eps, z16, z32, B, Z, state, hparams, stream, kld_part)
        "combine_reparam: ks = 0": lambda: C.combine_reparam(f(ks * 2 * n), 0, None, f(2 * n), f(n), h(n), None, B, Z,
                                                             S, H, 0, f(B)),
        "combine_reparam: B = 0": lambda: C.combine_reparam(f(ks * 2 * n), ks, None, f(2 * n), f(n), h(n), None, 0, Z,
                                                            S, H, 0, f(B)),
        "combine_reparam: Z = 0": lambda: C.combine_reparam(f(ks * 2 * n), ks, None, f(2 * n), f(n), h(n), None, B, 0,
                                                            S, H, 0, f(B)),
        "combine_reparam: ws short": lambda: C.combine_reparam(f(ks * 2 * n - 1), ks, None, f(2 * n), f(n), h(n), None,
                                                               B, Z, S, H, 0, f(B)),
        "combine_reparam: kld_part short": lambda: C.combine_reparam(f(ks * 2 * n), ks, None, f(2 * n), f(n), h(n),
                                                                     None, B, Z, S, H, 0, f(B - 1)),
        "combine_reparam: bias short": lambda: C.combine_reparam(f(ks * 2 * n), ks, f(2 * Z - 1), f(2 * n), f(n), h(n),
                                                                 None, B, Z, S, H, 0, f(B)),
        "combine_reparam: eps bf16": lambda: C.combine_reparam(f(ks * 2 * n), ks, None, f(2 * n), h(n), h(n), None, B,
                                                               Z, S, H, 0, f(B)),
        # combine_reparam_bwd(ws, ks, mulv, eps, dmulv, dmulv16, dz, B, Z, hparams, state)
        "combine_reparam_bwd: ks = 0": lambda: C.combine_reparam_bwd(f(ks * n), 0, f(2 * n), f(n), f(2 * n), None, None,
                                                                     B, Z, H),
        "combine_reparam_bwd: mulv short": lambda: C.combine_reparam_bwd(f(ks * n), ks, f(2 * n - 1), f(n), f(2 * n),
                                                                         None, None, B, Z, H),
        "combine_reparam_bwd: eps short": lambda: C.combine_reparam_bwd(f(ks * n), ks, f(2 * n), f(n - 1), f(2 * n),
                                                                        None, None, B, Z, H),
        "combine_reparam_bwd: dz short": lambda: C.combine_reparam_bwd(f(ks * n), ks, f(2 * n), f(n), f(2 * n), None,
                                                                       f(n - 1), B, Z, H),
        "combine_reparam_bwd: Z = 0": lambda: C.combine_reparam_bwd(f(ks * n), ks, f(2 * n), f(n), f(2 * n), None, None,
                                                                    B, 0, H),
        # loss_finalize2(bce_part, nb, kld_part, nk, state, hparams, advance_cursor)
        "loss_finalize2: partials short": lambda: C.loss_finalize2(f(3), 4, f(3), 3, S, H, True),
        "loss_finalize2: state short": lambda: C.loss_finalize2(f(3), 3, f(3), 3, S[:64], H, True),
        # adam_cast(P, G, m, v, w16, segs, nseg, state, hparams, do_adam)
        "adam_cast: total % 4": lambda: C.adam_cast(f(6), f(6), f(6), f(6), h(6), S, 0, S, H, False),
        "adam_cast: w16 f32": lambda: C.adam_cast(f(8), f(8), f(8), f(8), f(8), S, 0, S, H, False),
        "adam_cast: G short": lambda: C.adam_cast(f(8), f(4), f(8), f(8), h(8), S, 0, S, H, False),
        "step_begin: state short": lambda: C.step_begin(S[:64], H),
    }
    before = st.read_state(False)
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"accepted: {name}")   # not a RuntimeError: reported under the violation's name
    torch.cuda.synchronize()
    assert st.read_state(False) == before


def test_zz_report_largest_ratios():
    """Not a check of its own: prints the largest error/bound ratio each kernel output reached in this run."""
    for name in sorted(SEEN):
        print(f"MAXRATIO {name} {SEEN[name]:.4g}")
