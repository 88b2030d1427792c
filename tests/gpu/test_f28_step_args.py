"""The fused 28x28 step kernel's buffer pointers (csrc/kernels/conv28_pair.h
``kptr``): every pointer of the paired body is read from the kernel-argument
segment where it is used and advanced to its sample there, and the one solo
body of ``f28_step_k`` reads its arguments the same way.

What can go wrong is a pointer: a wrong per-sample stride, a null argument
that stopped being null, the M-dependent offset of a tail batch. So every
buffer the step kernel writes -- not only the parameters -- is compared
bitwise against the unchanged two-launch solo kernels (``f28_fwd_k`` +
``f28_bwd_k``, ``f28_merge = False``) in the same process. Whole buffers are
compared, rows past M included: a store through a wrongly advanced pointer
lands in a row the reference left alone. The enc2 bias partials are the one
buffer whose layout differs by form (the pair writes ``[2][M][64]``, the solo
body zeroes the second row): they are compared by their per-sample sums
row 0 + row 1, the order the finalize adds them in.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 2  # whole batches in the index list (+ the tail batch, when there is one)


def _trainer(B, **kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=B, image=28, device=torch.device("cuda"), backend="hip", seed=3, **kw)
    assert tr.f28
    return tr


@functools.lru_cache(maxsize=None)
def _data(B, tail):
    g = torch.Generator().manual_seed(100 * B + tail)
    n = NB * B + tail
    return torch.rand(n, 784, generator=g).cuda(), torch.randperm(n, generator=g).to(torch.int32).cuda()


def _buffers(tr, M):
    """Every buffer the step kernel writes, cloned (after a step of M samples)."""
    torch.cuda.synchronize()
    B = tr.B
    fb, fp = tr.f28_bias, tr.f28_part
    db2 = fb[B * 3168:B * 3168 + 2 * M * 64].view(2, M, 64)
    out = {"xb": tr.xb, "a1": tr.acts["enc1"], "a2": tr.acts["enc2"], "mulv": tr.mulv, "eps": tr.eps, "z16": tr.z16,
           "d0": tr.acts["dec_fc"], "d1": tr.acts["dec1"], "dlog32": tr.dlog32,
           "gd1": tr.gacts["dec1"], "gd0": tr.gacts["dec_fc"], "dbd": fb[:B * 3136], "dmulv": tr.dmulv,
           "dmulv16": tr.dmulv16, "ga2": tr.gacts["enc2"], "ga1": tr.gacts["enc1"],
           "db1": fb[B * 3296:], "db2.sum": db2[0] + db2[1], "db3": fb[B * 3136:B * 3168],
           "bce": fp[:B], "kld": fp[B:2 * B], "db4": fp[2 * B:]}
    return {k: v.clone() for k, v in out.items()}


def _run(B, tail, form, graphs=False, stamps=False, epi=True):
    """One trainer through: the tail batch FIRST (fresh, all-zero buffers, so
    rows >= M show any stray store), two whole batches, then a snapshot of
    every buffer after each, and of the training state at the end.
    form: "two" (f28_fwd_k + f28_bwd_k), "pair", "late" (every partner arrives
    late: leaders run the solo body, partners exit), "nopair" (grid M)."""
    X, idx = _data(B, tail)
    tr = _trainer(B, use_graphs=graphs, graph_steps=3)
    tr.f28_merge = form != "two"
    tr.f28_pair = form in ("pair", "late")
    tr.f28_pair_delay_us = 30 if form == "late" else 0
    tr.f28_epi_adam = epi
    st = None
    if stamps:
        st = torch.zeros(2 * B * 16, dtype=torch.int64, device="cuda")
        tr.f28_stamps = (st, None)
    tr.bind_train_data(X, idx)
    nb = NB + (1 if tail else 0)  # batches in the index list: the cursor must never leave it
    res = {}
    if tail:
        tr.set_cursor(NB, nb)
        tr.train_steps(1, M=tail)
        res["tail"] = _buffers(tr, tail)
        if st is not None:
            torch.cuda.synchronize()
            res["tail.slot15"] = st.view(2 * B, 16)[:, 15].cpu().clone()
    tr.set_cursor(0, nb)
    tr.train_steps(1)
    res["first"] = _buffers(tr, B)
    res["adamc"] = tr.f28_adamc.clone()
    if st is not None:
        res["slot15"] = st.view(2 * B, 16)[:, 15].cpu().clone()
        res["stamped"] = bool((st.view(2 * B, 16)[:, 2:15] != 0).any())
    tr.train_steps(1)
    res["whole"] = _buffers(tr, B)
    nsteps = 2 + (1 if tail else 0)
    assert tr.health_error() is None
    res["state"] = {"loss": torch.from_numpy(tr.loss_history()[:nsteps].copy()), "params": tr.params.clone(),
                    "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone()}
    res["pairw"] = int(tr.f28_pairw.abs().sum())
    res["xg"] = int(tr.f28_xg.abs().sum())
    res["err"] = int(tr.f28_err.item())
    return res


@functools.lru_cache(maxsize=None)
def _reference(B, tail):
    """The two-launch solo kernels: computed once per shape, shared, never changed."""
    return _run(B, tail, "two")


def _assert_same(got, ref, what):
    bad = {k: float((got[k].float() - ref[k].float()).abs().max()) for k in ref if not torch.equal(got[k], ref[k])}
    assert not bad, (what, bad)


def _assert_equals_reference(res, B, tail):
    ref = _reference(B, tail)
    for snap in ("tail", "first", "whole", "state"):
        if snap in ref:
            _assert_same(res[snap], ref[snap], snap)
    assert res["pairw"] == 0 and res["xg"] == 0 and res["err"] == 0


# B = 8: both workgroups of a pair (blocks n, n + 8) on one XCD, the `near` hand-offs;
# B = 3: M % 8 != 0, pairs (n, n + 3) across XCDs; (8, 5): an epoch of 8 k + 5 rows, tail batch M = 5 < B
SHAPES = [(8, 0), (3, 0), (8, 5)]


@pytest.mark.parametrize("B,tail", SHAPES)
def test_paired_step_writes_every_buffer_as_the_two_launches(native_ext, B, tail):
    res = _run(B, tail, "pair", stamps=True)
    _assert_equals_reference(res, B, tail)
    modes = res["slot15"] & 15
    assert sorted(modes.tolist()) == [1] * B + [2] * B, modes  # every sample ran as a pair: role 0 + role 1
    near = int(((res["slot15"] >> 4) & 1).sum())
    print(f"B={B}: {near} of {2 * B} workgroups took the near hand-off")
    if B % 8 == 0:
        assert near > 0, "no same-XCD pair took the near hand-off"


def test_tail_batch_last_sample_and_rows_past_it(native_ext):
    """M = 5 < B = 8 as the first step of a fresh trainer: the last sample
    n = M - 1 is written (and equal), rows M .. B - 1 of every per-sample
    buffer are still zero, and the second enc2-bias row sits at M * 64."""
    B, M = 8, 5
    got, ref = _run(B, M, "pair")["tail"], _reference(B, M)["tail"]
    for k, v in got.items():
        if k == "db2.sum":
            rows, rref = v, ref[k]
        else:
            rows, rref = v.view(B, -1), ref[k].view(B, -1)
            assert not rows[M:].any(), f"{k}: a row past M was written"
        assert torch.equal(rows[M - 1], rref[M - 1]), f"{k}: sample M - 1 differs"
        assert rows[M - 1].any(), f"{k}: sample M - 1 was not written"


@pytest.mark.parametrize("B,tail", [(8, 5), (3, 0)])
def test_late_partner_and_unpaired_launch_share_the_solo_body(native_ext, B, tail):
    """Leaders whose partners come late claim their samples solo (the partners
    exit); a launch without pairs enters the same solo body. Both equal the
    paired form and the two launches, and leave the pairing words clean."""
    late = _run(B, tail, "late", stamps=True)
    modes = late["slot15"][:2 * B] & 15
    assert sorted(modes.tolist()) == [0] * B + [3] * B, modes  # leaders solo, partners exit
    nopair = _run(B, tail, "nopair")
    for res in (late, nopair):
        _assert_equals_reference(res, B, tail)
    assert torch.equal(late["adamc"], nopair["adamc"])


def test_stamps_on_and_off_give_the_same_outputs(native_ext):
    on, off = _run(8, 5, "pair", stamps=True), _run(8, 5, "pair", stamps=False)
    assert on["stamped"]
    for snap in ("tail", "first", "whole", "state"):
        _assert_same(on[snap], off[snap], snap)
    _assert_equals_reference(off, 8, 5)


def test_adam_constants_handed_over_and_parameters_after_one_step(native_ext):
    """With the Adam epilogues on, the step kernel hands the step's constants
    over through PairCtl.adamc (read from the argument segment by the one
    hand-off thread): after ONE step the parameters are the two-launch
    tail's, in every form, and every form hands over the same constants."""
    B = 8
    X, idx = _data(B, 0)
    res = {}
    for form in ("two", "pair", "late", "nopair"):
        tr = _trainer(B, use_graphs=False)
        tr.f28_merge = form != "two"
        tr.f28_pair = form in ("pair", "late")
        tr.f28_pair_delay_us = 30 if form == "late" else 0
        assert tr.f28_epi_adam
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, NB)
        tr.train_steps(1)
        torch.cuda.synchronize()
        if form != "two":
            assert tr._epi_plan28(tr._plan28(B)) is not None  # the epilogue form is what ran
            assert tr.f28_adamc.any()
        res[form] = {"params": tr.params.clone(), "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone(),
                     "w16": tr.w16.clone(), "adamc": tr.f28_adamc.clone()}
    for form in ("pair", "late", "nopair"):
        _assert_same({k: v for k, v in res[form].items() if k != "adamc"},
                     {k: v for k, v in res["two"].items() if k != "adamc"}, form)
        assert torch.equal(res[form]["adamc"], res["pair"]["adamc"])


def test_captured_graph_replayed_twice_equals_eager(native_ext):
    """A 3-step captured graph replayed twice (6 steps) against 6 eager steps:
    the argument segment is part of the captured launch."""
    B = 8
    X, idx = _data(B, 0)
    res = []
    for graphs in (False, True):
        tr = _trainer(B, use_graphs=graphs, graph_steps=3)
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, NB)
        tr.train_steps(6)
        bufs = _buffers(tr, B)
        bufs.update(loss=torch.from_numpy(tr.loss_history()[:6].copy()), params=tr.params.clone(),
                    exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone())
        assert int(tr.f28_pairw.abs().sum()) == 0 and int(tr.f28_err.item()) == 0
        res.append(bufs)
    _assert_same(res[1], res[0], "graph vs eager")


@pytest.mark.parametrize("want_recon", [True, False])
def test_eval_forward_paired_and_solo(native_ext, want_recon):
    """Eval forward (train = 0): the activation pointers, `stamps` and -- without
    a reconstruction -- `recon` are null arguments, and must stay null at their
    points of use. The paired step kernel against the solo f28_fwd_k: same
    loss, partials and reconstruction, no activation buffer touched."""
    B = 8
    X, idx = _data(B, 5)
    res = []
    for pair in (False, True):
        tr = _trainer(B, use_graphs=False)
        tr._eval_pair = pair
        tr.recon.fill_(-1.0)
        total, first = tr.evaluate(X, idx, want_first_recon=want_recon)
        torch.cuda.synchronize()
        assert np.isfinite(total) and (first is not None) == want_recon
        for k in ("enc1", "enc2", "dec_fc", "dec1"):
            assert not tr.acts[k].any(), f"eval wrote the {k} activations"
        assert not tr.dlog32.any()
        assert int(tr.f28_pairw.abs().sum()) == 0 and int(tr.f28_xg.abs().sum()) == 0 and int(tr.f28_err.item()) == 0
        res.append({"total": torch.tensor(total, dtype=torch.float64), "part": tr.f28_part.clone(),
                    "recon": tr.recon.clone(), **({"first": first.clone()} if want_recon else {})})
    _assert_same(res[1], res[0], "eval pair vs solo")
