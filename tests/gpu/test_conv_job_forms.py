"""The recorded (job) form of an op against its stand-alone launch, bit for bit,
for the ops that had no such comparison: colsum, loss_finalize2, grad_finalize
and wtrans. Both forms are built by ONE host builder per op (csrc/kernels/
conv_igemm.hip, conv_bf16.hip, conv_thin.hip) and run the same device body, so
every output must be equal, not close. Inputs are the smallest of each op's
stand-alone test in tests/gpu/test_conv_small_kernels.py. A single job runs in a
jobs_multi_k launch; wtrans, which that kernel does not dispatch, runs next to a
finalize job in the jobs_k<JFinalize, JWtrans> launch.

The edges on which the two forms differ on purpose are pinned at the end."""
import pytest
import torch

from tests import conv_small_checker as ck

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


def _state(C, step=7):
    hp = ck.ADAM_SETS["default"]
    st = C.TrialState(0)
    st.set_hparams(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], 1.0, hp["grad_scale"], 0,
                   hp["decoupled"], lr_warmup_steps=hp["lr_warmup_steps"], kl_anneal_steps=0)
    st.set_step(False, step)
    return st


def _run_alone(C, job):
    """`job` by itself in one jobs_multi_k launch."""
    assert job.kind > 0 and not job.has_post
    img, grid = C.pack_jobs_multi([job])
    assert grid == job.nblk
    C.launch_jobs_multi(img.to(DEV), grid)
    torch.cuda.synchronize()


def test_colsum_job(native_ext):
    C = native_ext
    M, N, rows_per = 9, 8, 4   # three row blocks, the last one partial
    G = torch.randint(-8, 9, (M, N), generator=ck.gen(M)).to(BF16).to(DEV)
    gy = -(-M // rows_per)
    alone, fused = (torch.full((gy * N + N,), float("nan"), device=DEV) for _ in range(2))
    C.colsum(G, M, N, rows_per, alone)
    job = C.Job()
    C.colsum(G, M, N, rows_per, fused, job=job)
    assert job.nblk == gy
    _run_alone(C, job)
    assert bool(torch.isfinite(alone[:gy * N]).all()) and bool(torch.isnan(alone[gy * N:]).all())
    assert torch.equal(alone[:gy * N], fused[:gy * N]) and bool(torch.isnan(fused[gy * N:]).all())


@pytest.mark.parametrize("advance_step", [False, True])
def test_loss_finalize2_job(advance_step, native_ext):
    C = native_ext
    nb, nk = 3, 2
    g = ck.gen(nb)
    bce = torch.randint(0, 9, (nb,), generator=g).float().to(DEV)
    kld = torch.randint(0, 9, (nk,), generator=g).float().to(DEV)
    got = []
    for as_job in (False, True):
        st = _state(C)
        st.set_cursor(False, 2, 4)
        if as_job:
            job = C.Job()
            C.loss_finalize2(bce, nb, kld, nk, st.train_state, st.hparams, True, job=job, advance_step=advance_step)
            assert job.nblk == 1
            _run_alone(C, job)
        else:
            C.loss_finalize2(bce, nb, kld, nk, st.train_state, st.hparams, True, advance_step=advance_step)
            torch.cuda.synchronize()
        got.append((list(st.read_state(False)), st.loss_history(False).clone(), st.train_state.cpu().clone()))
    (rs0, h0, raw0), (rs1, h1, raw1) = got
    assert rs0[0] == (8 if advance_step else 7) and rs0[1] == 3   # the step and the cursor moved as asked
    assert rs0 == rs1 and torch.equal(h0, h1) and torch.equal(raw0, raw1)   # ring, cursor, step: all of the state


def _finalize_case(numel, ns):
    slab = (3.0 * torch.randn(ns, numel, generator=ck.gen(3))).to(DEV)
    p, _, m, v = ck.adam_inputs(numel, seed=4)
    bufs = [p.to(DEV), torch.full((numel,), float("nan"), device=DEV), m.to(DEV), v.to(DEV),
            torch.full((numel,), ck.BF16_FILL, dtype=BF16, device=DEV)]
    return slab, bufs


# one unit of at most 256 elements (one element per thread group, split slabs);
# one above 256 (four per thread) whose tail is 906 % 4 = 2 elements
@pytest.mark.parametrize("do_adam", [False, True])
@pytest.mark.parametrize("numel", [250, 906])
def test_grad_finalize_job(numel, do_adam, native_ext):
    C = native_ext
    ns = 3
    slab, alone = _finalize_case(numel, ns)
    fused = [t.clone() for t in alone]
    segs = C.make_grad_segs([[0, numel, slab.data_ptr(), ns, 0, 0, 0, 0, -1]], 0)
    U = C.make_grad_units([[0, 0, numel]], 0)
    st = _state(C, step=1000)
    C.grad_finalize(*alone, segs, U, 1, st.train_state, st.hparams, do_adam)
    job = C.Job()
    C.grad_finalize(*fused, segs, U, 1, st.train_state, st.hparams, do_adam, job=job)
    assert job.nblk == 1
    _run_alone(C, job)
    for name, a, f in zip(("P", "G", "m", "v", "w16"), alone, fused):
        assert torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32),
                           f.view(torch.int16 if f.dtype == BF16 else torch.int32)), name
    # the launch did something: the gradient is stored (plain) or consumed into P and w16 (Adam)
    assert bool(torch.isnan(alone[1]).all()) == do_adam
    assert bool((alone[4].float() == ck.BF16_FILL).all()) == (not do_adam)


def test_finalize_and_wtrans_jobs_in_one_launch(native_ext):
    """jobs_k<JFinalize, JWtrans>: the finalize of one segment next to the
    transposed copy of another (the two never touch the same weights in one
    launch), against the two stand-alone kernels."""
    C = native_ext
    nfin, ns = 906, 3
    co, k, s, ci = 72, 2, 2, 72            # per tap 2 x 2 tiles of 64 x 64: a full one, and partial in co, in ci, in both
    woff, wn = 1024, co * k * k * ci
    total = woff + wn
    slab = (3.0 * torch.randn(ns, nfin, generator=ck.gen(5))).to(DEV)
    segs = C.make_grad_segs([[0, nfin, slab.data_ptr(), ns, 0, 0, 0, 0, -1],
                             [woff, wn, 0, 1, co, k, s, ci, 0]], 0)
    U = C.make_grad_units([[0, 0, nfin]], 0)
    tr = [[1, tap, co0, ci0] for tap in range(k * k) for co0 in range(0, co, 64) for ci0 in range(0, ci, 64)]
    T = C.make_tr_units(tr, 0)
    p, _, m, v = ck.adam_inputs(total, seed=6)

    def bufs():
        w16 = p.to(BF16).to(DEV)
        return ([p.to(DEV), torch.full((total,), float("nan"), device=DEV), m.to(DEV), v.to(DEV), w16],
                torch.full((wn + 8,), ck.BF16_FILL, dtype=BF16, device=DEV))

    st = _state(C, step=1000)
    alone, alone_t = bufs()
    C.grad_finalize(*alone, segs, U, 1, st.train_state, st.hparams, True)
    C.wtrans(alone[4], alone_t, segs, T, len(tr))
    fused, fused_t = bufs()
    jf, jw = C.Job(), C.Job()
    C.grad_finalize(*fused, segs, U, 1, st.train_state, st.hparams, True, job=jf)
    C.wtrans(fused[4], fused_t, segs, T, len(tr), job=jw)
    assert (jf.nblk, jw.nblk) == (1, len(tr)) and jf.kind > 0 and jw.kind > 0
    assert C.launch_jobs([jf, jw]), "no fused kernel for a finalize and a wtrans job"
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16 if t.dtype == BF16 else torch.int32)
    for name, a, f in zip(("P", "G", "m", "v", "w16"), alone, fused):
        assert torch.equal(bits(a), bits(f)), name
    assert torch.equal(bits(alone_t), bits(fused_t))
    # every element of the copy was written, nothing behind it, and it is the parity-ordered transpose
    from multidisttorch_amd.ops.conv_layout import parity_transpose

    assert bool((alone_t[wn:].float() == ck.BF16_FILL).all())
    w = alone[4][woff:].view(co, k, k, ci)
    assert torch.equal(alone_t[:wn], parity_transpose(w, s).reshape(-1))


# ------------------------------------------------- where the two forms differ ----
def test_no_units_is_a_no_op_when_launched_and_an_error_when_recorded(native_ext):
    C = native_ext
    numel = 8
    slab, bufs = _finalize_case(numel, 1)
    before = [t.clone() for t in bufs]
    segs = C.make_grad_segs([[0, numel, slab.data_ptr(), 1, 8, 1, 1, 1, 0]], 0)
    U, T = C.make_grad_units([], 0), C.make_tr_units([], 0)
    st = _state(C)
    w16t = torch.full((numel,), ck.BF16_FILL, dtype=BF16, device=DEV)
    C.grad_finalize(*bufs, segs, U, 0, st.train_state, st.hparams, True)
    C.wtrans(bufs[4], w16t, segs, T, 0)
    torch.cuda.synchronize()
    for a, b in zip(before, bufs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert bool((w16t.float() == ck.BF16_FILL).all())
    job = C.Job()
    with pytest.raises(RuntimeError, match="job_finalize"):
        C.grad_finalize(*bufs, segs, U, 0, st.train_state, st.hparams, True, job=job)
    assert job.kind == 0
    with pytest.raises(RuntimeError, match="job_wtrans"):
        C.wtrans(bufs[4], w16t, segs, T, 0, job=job)
    assert job.kind == 0


def test_thin_conv_without_a_kernel_raises_when_launched_and_records_kind_0(native_ext):
    C = native_ext
    N, H, CO = 1, 8, 8   # CO = 8: neither 16, 32 nor 64
    d = [N, H, H, 1, H // 2, H // 2, CO, 4, 4, 2, 1]
    M = N * (H // 2) ** 2
    X = torch.zeros(N * H * H, dtype=BF16, device=DEV)
    Wf = torch.zeros(CO * 16, device=DEV)
    y16 = torch.full((M * CO,), ck.BF16_FILL, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match=r"thin_conv failed \(2\)"):
        C.thin_conv(X, Wf, d, None, False, y16)
    job = C.Job()
    C.thin_conv(X, Wf, d, None, False, y16, job=job)
    assert job.kind == 0 and job.nblk == 1
    torch.cuda.synchronize()
    assert bool((y16.float() == ck.BF16_FILL).all())
