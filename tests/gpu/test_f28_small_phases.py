"""The paired 28x28 step's small phases after their schedule changed
(csrc/kernels/conv28_pair.h): the step's scalars (``step``, the free-bits
floor, the KL weight, the Philox seed) are loaded once at the top of the
paired body and left in LDS words, eps is drawn in P3, each wave publishes its
eight head sums in one store, the XCD id is polled by a second wave, the
loss partials are summed by a thread of wave 7 after its Q1 work, the dec1
bias partials are summed in X5 + Q4 by two otherwise idle waves (the barrier
in front of X4 is gone), and Q4 forms its KL terms before it polls.

None of that may change a bit, so every buffer the kernel writes -- the
loss, KL and bias partials (``bce``, ``kld``, ``db4``, ``db3``), ``mulv``,
``eps`` and ``z16`` among them -- is compared bitwise, whole buffers with the
rows past M, against the two-launch solo kernels (``f28_fwd_k`` +
``f28_bwd_k``) in the same process. All trainers run with a free-bits floor
above zero, so the floor's LDS word takes part in P4 and Q4.

What is specific to this change: the hoisted words must be re-read on every
launch (the host moves ``step``, the floor and the seed between launches; a
captured graph advances ``step`` inside a replay), LDS words 24 .. 29 of the
scratch row must not collide with anything, and the moved sums must still
see their inputs (the loss sums in eval launches, which return before Q1;
the dec1 bias sums of every own channel, for both roles).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 2     # whole batches in the index list (+ the tail batch, when there is one)
FB = 0.02  # free-bits floor of every trainer here (nats per latent element)


def _trainer(B, **kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=B, image=28, device=torch.device("cuda"), backend="hip", seed=5, free_bits=FB, **kw)
    assert tr.f28
    return tr


@functools.lru_cache(maxsize=None)
def _data(B, tail):
    g = torch.Generator().manual_seed(1000 * B + tail)
    n = NB * B + tail
    return torch.rand(n, 784, generator=g).cuda(), torch.randperm(n, generator=g).to(torch.int32).cuda()


def _form(tr, form):
    """"two": f28_fwd_k + f28_bwd_k; "pair"; "late": every partner arrives late (leaders run the
    solo body, partners exit); "nopair": grid M."""
    tr.f28_merge = form != "two"
    tr.f28_pair = form in ("pair", "late")
    tr.f28_pair_delay_us = 30 if form == "late" else 0


def _buffers(tr, M):
    """Every buffer the step kernel writes, cloned (after a step of M samples)."""
    torch.cuda.synchronize()
    B = tr.B
    fb, fp = tr.f28_bias, tr.f28_part
    db2 = fb[B * 3168:B * 3168 + 2 * M * 64].view(2, M, 64)  # [2][M][64] paired, second row zero solo
    out = {"xb": tr.xb, "a1": tr.acts["enc1"], "a2": tr.acts["enc2"], "mulv": tr.mulv, "eps": tr.eps, "z16": tr.z16,
           "d0": tr.acts["dec_fc"], "d1": tr.acts["dec1"], "dlog32": tr.dlog32,
           "gd1": tr.gacts["dec1"], "gd0": tr.gacts["dec_fc"], "dbd_part": fb[:B * 3136], "dmulv": tr.dmulv,
           "dmulv16": tr.dmulv16, "ga2": tr.gacts["enc2"], "ga1": tr.gacts["enc1"],
           "db1_part": fb[B * 3296:], "db2_part.sum": db2[0] + db2[1], "db3_part": fb[B * 3136:B * 3168],
           "bce_part": fp[:B], "kld_part": fp[B:2 * B], "db4_part": fp[2 * B:]}
    return {k: v.clone() for k, v in out.items()}


def _state(tr, nsteps):
    return {"loss": torch.from_numpy(tr.loss_history()[:nsteps].copy()), "params": tr.params.clone(),
            "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone()}


def _run(B, tail, form, stamps=False):
    """The tail batch FIRST (fresh all-zero buffers: rows >= M show a stray
    store), a whole batch, then the host moves `step`, the free-bits floor and
    the seed, and a last whole batch runs: a snapshot of every buffer after each."""
    X, idx = _data(B, tail)
    tr = _trainer(B, use_graphs=False)
    _form(tr, form)
    st = None
    if stamps:
        st = torch.zeros(2 * B * 16, dtype=torch.int64, device="cuda")
        tr.f28_stamps = (st, None)
    tr.bind_train_data(X, idx)
    nb = NB + (1 if tail else 0)
    res = {}
    if tail:
        tr.set_cursor(NB, nb)
        tr.train_steps(1, M=tail)
        res["tail"] = _buffers(tr, tail)
    tr.set_cursor(0, nb)
    tr.train_steps(1)
    res["first"] = _buffers(tr, B)
    if st is not None:
        res["slot15"] = st.view(2 * B, 16)[:, 15].cpu().clone()
        res["stamped"] = bool((st.view(2 * B, 16)[:, 2:15] != 0).any())
    # host-side change between two launches: every hoisted word moves
    tr.set_step(1000)
    tr.set_hparams(free_bits=0.3)
    tr.seed = 77
    tr._push_hparams()
    tr.train_steps(1)
    res["moved"] = _buffers(tr, B)
    assert tr.health_error() is None
    res["state"] = _state(tr, 2 + (1 if tail else 0))
    res["clean"] = (int(tr.f28_pairw.abs().sum()), int(tr.f28_xg.abs().sum()), int(tr.f28_err.item()))
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
    for snap in ("tail", "first", "moved", "state"):
        if snap in ref:
            _assert_same(res[snap], ref[snap], snap)
    assert res["clean"] == (0, 0, 0), res["clean"]


def test_host_moved_step_floor_and_seed_reach_the_reference(native_ext):
    """The premise of the `moved` snapshots: in the reference itself the moved
    seed and step change eps, and the raised floor changes the KL partials."""
    ref = _reference(2, 0)
    assert not torch.equal(ref["first"]["eps"], ref["moved"]["eps"])
    assert not torch.equal(ref["first"]["kld_part"], ref["moved"]["kld_part"])
    for k in ("bce_part", "kld_part", "db4_part", "db3_part", "mulv", "eps", "z16"):
        assert ref["moved"][k].float().abs().sum() > 0, k


# B = 2: pairs (n, n + 2), the smallest paired launch; B = 3: M % 8 != 0, pairs (n, n + 3) across XCDs;
# B = 8: both workgroups of a pair (blocks n, n + 8) on one XCD, the `near` hand-offs; (8, 5): tail batch M = 5 < B
@pytest.mark.parametrize("B,tail", [(2, 0), (3, 0), (8, 5)])
def test_paired_step_equals_the_two_launches(native_ext, B, tail):
    res = _run(B, tail, "pair", stamps=True)
    _assert_equals_reference(res, B, tail)
    modes = res["slot15"] & 15
    assert sorted(modes.tolist()) == [1] * B + [2] * B, modes  # every sample ran as a pair: role 0 + role 1
    near = int(((res["slot15"] >> 4) & 1).sum())
    print(f"B={B}: {near} of {2 * B} workgroups took the near hand-off")
    if B % 8 == 0:
        assert near > 0, "no same-XCD pair took the near hand-off"
    if B == 3:
        assert near < 2 * B, "every pair of B = 3 was near: no cross-XCD pair ran"


def test_tail_batch_rows_past_m_untouched(native_ext):
    B, M = 8, 5
    got, ref = _run(B, M, "pair")["tail"], _reference(B, M)["tail"]
    for k, v in got.items():
        if k == "db2_part.sum":
            rows, rref = v, ref[k]
        else:
            rows, rref = v.view(B, -1), ref[k].view(B, -1)
            assert not rows[M:].any(), f"{k}: a row past M was written"
        assert torch.equal(rows[M - 1], rref[M - 1]), f"{k}: sample M - 1 differs"
        assert rows[M - 1].any(), f"{k}: sample M - 1 was not written"


@pytest.mark.parametrize("form", ["late", "nopair"])
def test_late_partner_and_unpaired_forms(native_ext, form):
    res = _run(8, 5, form, stamps=form == "late")
    _assert_equals_reference(res, 8, 5)
    if form == "late":
        modes = res["slot15"][:16] & 15
        assert sorted(modes.tolist()) == [0] * 8 + [3] * 8, modes  # leaders solo, partners exit


def test_stamps_on_and_off(native_ext):
    on, off = _run(8, 5, "pair", stamps=True), _run(8, 5, "pair", stamps=False)
    assert on["stamped"]
    for snap in ("tail", "first", "moved", "state"):
        _assert_same(on[snap], off[snap], snap)
    _assert_equals_reference(off, 8, 5)


def test_three_step_graph_replayed_twice(native_ext):
    """A 3-step captured graph replayed twice (6 steps) against 6 eager steps
    of the two-launch kernels: `step` advances inside a replay, so the tags and
    the hoisted words of launch k + 1 must be those the finalize of launch k left."""
    B = 8
    X, idx = _data(B, 0)
    res = []
    for graphs in (False, True):
        tr = _trainer(B, use_graphs=graphs, graph_steps=3)
        if not graphs:
            _form(tr, "two")
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, NB)
        tr.train_steps(6)
        bufs = _buffers(tr, B)
        bufs.update(_state(tr, 6))
        assert int(tr.f28_pairw.abs().sum()) == 0 and int(tr.f28_xg.abs().sum()) == 0 and int(tr.f28_err.item()) == 0
        res.append(bufs)
    _assert_same(res[1], res[0], "paired graph vs two-launch eager")


@pytest.mark.parametrize("want_recon", [True, False])
def test_eval_forward(native_ext, want_recon):
    """Eval (train = 0) returns before Q1: the loss partials, summed by a
    thread of wave 7 since this change, must still be written, and no
    activation buffer touched. Paired step kernel against the solo f28_fwd_k."""
    B = 8
    X, idx = _data(B, 5)
    res = []
    for pair in (False, True):
        tr = _trainer(B, use_graphs=False)
        tr._eval_pair = pair
        tr.recon.fill_(-1.0)
        tr.f28_part.fill_(-7.0)
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
    assert (res[1]["part"][:2 * B] != -7.0).all(), "a loss partial of the paired eval was not written"
