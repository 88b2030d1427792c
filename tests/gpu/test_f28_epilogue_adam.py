"""Adam in the weight-gradient epilogues of the fused 28x28 step's Linear
layers (MDT_F28_EPI_ADAM, conv_igemm_dev.h wgrad_epilogue_adam) on one MI355X.

The oracle is the two-launch tail of the same build in the same process
(``f28_epi_adam = False``): every weight gradient writes its partial slab and
the finalize launch applies Adam to all of them. Neither form sums anything in
another order, and the step kernel's hand-off (adam_consts_next) rounds the
Adam constants as step_advance + adam_consts_block do, so every comparison is
bitwise: parameters, both moments, the bf16 weight copies, the loss ring, the
gathered next batch and the weight average.

64 x 3136 and 3136 x 32 divide the 64x64 / 64x32 tiles exactly, so the cases
are about the m-loop (B = 128: two full m-tiles, B = 72: a partial second one,
B = 8 with a tail of 5: one partial tile) and about constants that differ
every step: lr warm-up and cosine decay, an lr change, a host step move,
weight decay of both kinds, the weight average.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 3  # whole batches in the index list (+ one tail batch)


def _trainer(B, epi, **kw):
    from multidisttorch_amd.hpo.schedule import Schedule
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    kw.setdefault("schedule", Schedule(lr_warmup_steps=3, lr_decay="cosine", lr_decay_steps=60, lr_min_ratio=0.1))
    tr = ConvVaeTrainer(batch_size=B, image=28, device=torch.device("cuda"), backend="hip", seed=4, lr=2e-3,
                        betas=(0.85, 0.97), ema_decay=0.9, **kw)
    assert tr.f28 and tr.f28_merge
    tr.f28_epi_adam = epi
    return tr


def _data(B, tail, seed):
    g = torch.Generator().manual_seed(seed)
    n = NB * B + tail
    X = torch.rand(n, 784, generator=g).cuda()
    idx = torch.randperm(n, generator=g).to(torch.int32).cuda()
    return X, idx


def _snap(tr, nloss):
    torch.cuda.synchronize()
    assert tr.health_error() is None
    return {"loss": torch.from_numpy(tr.loss_history()[:nloss].copy()), "params": tr.params.clone(),
            "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone(), "w16": tr.w16.clone(),
            "xn": tr.f28_xn.clone(), "xtag": tr.f28_xtag.clone(), "ema": tr.ema.clone()}


def _assert_same(got, ref):
    bad = {k: float((got[k].float() - ref[k].float()).abs().max()) for k in ref if not torch.equal(got[k], ref[k])}
    assert not bad, bad


def _run(tr, B, tail, X, idx):
    """11 steps: whole batches (graphs: one S = 3 graph + the S = 1 remainder),
    the tail batch, a host cursor move, an lr change, a host step move into
    the cosine part of the schedule."""
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, NB + 1)
    tr.train_steps(4)             # steps 1-4: warm-up (3 steps), then the first cosine step; cursor wraps at NB + 1
    tr.set_cursor(NB, NB + 1)
    tr.train_steps(1, M=tail)     # the tail batch
    tr.set_cursor(1, NB + 1)      # host cursor move
    tr.train_steps(2)
    tr.set_hparams(lr=7e-4)       # lr changes between two steps
    tr.train_steps(1)
    tr.set_step(40)               # host step move: beta^t, lr_t re-seeded by the host
    tr.set_cursor(0, NB + 1)
    tr.train_steps(3)
    return _snap(tr, 11)


# (B, tail, graphs, pair, pair_delay_us, weight_decay, decoupled)
CASES = [
    (128, 40, False, True, 0, 1e-2, False),
    (128, 40, True, True, 0, 1e-2, True),
    (128, 40, True, False, 0, 0.0, False),
    (128, 40, False, True, 30, 1e-2, True),   # late partners: the solo-claiming leader hands the constants over
    (72, 40, True, True, 0, 1e-2, False),
    (72, 40, False, False, 0, 1e-2, True),
    (8, 5, False, True, 0, 1e-2, False),
    (8, 5, True, True, 30, 0.0, False),
]


@pytest.mark.parametrize("B,tail,graphs,pair,delay,wd,decoupled", CASES)
def test_epilogue_adam_is_bitwise_the_finalize(native_ext, B, tail, graphs, pair, delay, wd, decoupled):
    X, idx = _data(B, tail, seed=B + tail)
    res = {}
    for epi in (False, True):
        tr = _trainer(B, epi, use_graphs=graphs, graph_steps=3, weight_decay=wd, decoupled_wd=decoupled)
        tr.f28_pair = pair
        tr.f28_pair_delay_us = delay
        res[epi] = _run(tr, B, tail, X, idx)
        if epi:  # the new form is what ran: both Linear layers plan one m-split at these sizes
            assert tr._epi_plan28(tr._plan28(B)) is not None and tr._epi_plan28(tr._plan28(tail)) is not None
        assert int(tr.f28_pairw.abs().sum()) == 0 and int(tr.f28_err.item()) == 0
    _assert_same(res[True], res[False])


def test_skip_adam_step_keeps_the_gradient_and_the_next_step_matches(native_ext):
    """f28_skip_adam for one step takes the two-launch form (the reduced
    gradient stays in ``grads``, nothing is updated); the step after it is the
    epilogue form again and equals the oracle."""
    B = 128
    X, idx = _data(B, 40, seed=77)
    res = {}
    for epi in (False, True):
        tr = _trainer(B, epi, use_graphs=False, weight_decay=1e-2)
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, NB + 1)
        tr.train_steps(2)
        before = tr.params.clone()
        tr.f28_skip_adam = True
        tr.train_steps(1)
        torch.cuda.synchronize()
        assert torch.equal(tr.params, before)
        grads = tr.grads.clone()
        assert float(grads.abs().max()) > 0
        tr.f28_skip_adam = False
        tr.train_steps(3)
        res[epi] = _snap(tr, 6)
        res[epi]["grads"] = grads
    _assert_same(res[True], res[False])


def test_no_schedule_and_switch_flipped_between_steps(native_ext):
    """No schedule (lr_t = lr_d * 1.0) and the switch flipped between steps of
    ONE trainer: the form is chosen per call, and a step of either form leaves
    the state the other form continues from."""
    B = 72
    X, idx = _data(B, 40, seed=5)
    res = {}
    for flip in (False, True):
        tr = _trainer(B, False, use_graphs=False, schedule=None)
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, NB + 1)
        for k in range(6):
            tr.f28_epi_adam = flip and k % 2 == 0
            tr.train_steps(1)
        res[flip] = _snap(tr, 6)
    _assert_same(res[True], res[False])


def test_two_m_splits_fall_back(native_ext):
    """B = 256: the planner gives the Linear weight gradients two m-splits, the
    plan has no epilogue form and the trainer runs the two-launch tail."""
    B = 256
    X, idx = _data(B, 40, seed=9)
    res = {}
    for epi in (False, True):
        tr = _trainer(B, epi, use_graphs=False, weight_decay=1e-2)
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, NB + 1)
        assert tr._epi_plan28(tr._plan28(B)) is None
        tr.train_steps(6)
        res[epi] = _snap(tr, 6)
    _assert_same(res[True], res[False])


def test_epilogue_form_writes_no_slab(native_ext):
    """The two Linear weight gradients of the epilogue form leave their partial
    slabs untouched (the other layers' slabs are written as before), so what
    the comparisons above saw was the new jobs, not the two-launch tail."""
    B = 128
    X, idx = _data(B, 40, seed=3)
    tr = _trainer(B, True, use_graphs=False)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, NB + 1)
    slabs = tr._plan28(B)["slabs"]
    for t, _ in slabs.values():
        t.fill_(123.0)
    tr.train_steps(2)
    torch.cuda.synchronize()
    for name, (t, _) in slabs.items():
        if not name.endswith(".weight"):
            continue
        untouched = bool((t == 123.0).all())
        assert untouched == (name.split(".")[0] in tr._EPI_ADAM28), name
