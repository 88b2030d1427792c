"""Weight averaging (``ema_decay``, csrc/kernels/ema.hip) on one MI355X: the two
kernels through their binding, every training-step form with and without the
average, graph replay, ``averaged_weights()``, checkpoints, and two replicas of
a conv trial whose comm-job tail is followed by ``ema_update``.

Oracle and bounds: tests/ema_cases.py (the definition in float64 on the float32
inputs; 16 times the float32 oracle's own error, floored by one float32 rounding
of the largest value that enters). Every check prints the achieved error next to
its bound; the last test prints the worst ratio of the module.
"""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import ema_cases as ec
from tests import mlp_checker as ck

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DECAY = 0.9
LR = 3e-3
TAIL = 5


def _dev():
    return torch.device("cuda", 0)


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


# ---------------------------------------------------------------- kernels through the binding
def _padded(v):
    buf = torch.full((v.numel() + ec.PAD,), ec.SENTINEL, dtype=torch.float32)
    buf[: v.numel()] = v
    return buf.to(_dev())


@pytest.mark.parametrize("n", ec.KERNEL_NS)
def test_ema_update_matches_the_float64_oracle(n, native_ext):
    C = _C()
    e0, p0 = ec.inputs(n)
    dp = _padded(p0)
    worst = 0.0
    for decay in ec.DECAYS:
        for t in ec.TS:
            e64, b = ec.bound(e0, p0, decay, t)
            outs = []
            for _ in range(2):
                de = _padded(e0)
                C.ema_update(de, dp, n, decay=decay, t=t)
                outs.append(de.cpu())
            assert torch.equal(outs[0], outs[1]), "not bitwise repeatable"
            worst = max(worst, ec.check(f"kernel n={n} decay={decay} t={t}", outs[0][:n], e64, b))
            assert bool((outs[0][n:] == ec.SENTINEL).all()), "wrote past n"
    assert torch.equal(dp.cpu()[:n], p0) and bool((dp.cpu()[n:] == ec.SENTINEL).all()), "p was written"
    print(f"ema kernel n={n}: worst error/bound {worst:.3f}")
    # e == p on entry: e == p bitwise on exit, whatever the factor
    for decay, t in ((0.9, 1), (0.999, 10 ** 6)):
        de = _padded(p0)
        C.ema_update(de, dp, n, decay=decay, t=t)
        assert torch.equal(de.cpu(), dp.cpu())


@pytest.mark.parametrize("n", ec.KERNEL_NS)
def test_arena_swap_is_bitwise_and_an_involution(n, native_ext):
    C = _C()
    a0, b0 = ec.inputs(n, seed=9)
    da, db = _padded(a0), _padded(b0)
    C.arena_swap(da, db, n)
    for got, want in ((da.cpu(), b0), (db.cpu(), a0)):
        assert torch.equal(got[:n], want) and bool((got[n:] == ec.SENTINEL).all())
    C.arena_swap(da, db, n)
    assert torch.equal(da.cpu()[:n], a0) and torch.equal(db.cpu()[:n], b0)


def test_buffers_off_the_16_byte_grid_take_the_scalar_form(native_ext):
    C = _C()
    n = 4099
    e0, p0 = ec.inputs(n)
    for off_e, off_p in ((1, 0), (0, 3), (2, 2)):
        be = torch.full((n + 16,), ec.SENTINEL, device=_dev())
        bp = torch.full((n + 16,), ec.SENTINEL, device=_dev())
        be[off_e: off_e + n] = e0.to(_dev())
        bp[off_p: off_p + n] = p0.to(_dev())
        ref = _padded(e0)
        C.ema_update(ref, _padded(p0), n, decay=0.9, t=81)
        C.ema_update(be[off_e:], bp[off_p:], n, decay=0.9, t=81)
        got = be.cpu()
        assert torch.equal(got[off_e: off_e + n], ref.cpu()[:n])      # bitwise the float4 form
        assert bool((got[:off_e] == ec.SENTINEL).all()) and bool((got[off_e + n:] == ec.SENTINEL).all())
        C.arena_swap(be[off_e:], bp[off_p:], n)
        assert torch.equal(bp.cpu()[off_p: off_p + n], ref.cpu()[:n]) and torch.equal(be.cpu()[off_e: off_e + n], p0)
        assert bool((bp.cpu()[off_p + n:] == ec.SENTINEL).all()) and bool((be.cpu()[off_e + n:] == ec.SENTINEL).all())


def test_step_and_decay_from_the_trial_state(native_ext):
    """The device form reads TrainState.step and HParams.ema_decay: bitwise the explicit (decay, t) form."""
    C = _C()
    n = 4099
    e0, p0 = ec.inputs(n)
    ts = C.TrialState(0)
    dp = _padded(p0)
    for decay, t in ((0.9, 1), (0.9, 80), (0.9, 81), (0.999, 10 ** 6), (0.0, 3)):
        ts.set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0, False, ema_decay=decay)
        ts.set_step(False, t)
        ts.set_step(True, t + 17)   # the eval state's step is not the one it reads
        a, b = _padded(e0), _padded(e0)
        C.ema_update(a, dp, n, state=ts.train_state, hparams=ts.hparams)
        C.ema_update(b, dp, n, decay=decay, t=t)
        assert torch.equal(a.cpu(), b.cpu()), (decay, t)
    with pytest.raises(ValueError):
        ts.set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0, False, ema_decay=1.0)


def test_domain_errors(native_ext):
    C = _C()
    e, p = torch.zeros(16, device=_dev()), torch.zeros(16, device=_dev())
    for kw in (dict(decay=1.0, t=1), dict(decay=-0.1, t=1), dict(decay=float("nan"), t=1), dict(decay=0.9, t=0)):
        with pytest.raises(ValueError):
            C.ema_update(e, p, 16, **kw)
    with pytest.raises(ValueError):
        C.ema_update(e, p, 0, decay=0.9, t=1)
    with pytest.raises(RuntimeError):
        C.ema_update(e, p, 17, decay=0.9, t=1)          # more elements than the buffers hold
    with pytest.raises(RuntimeError):
        C.ema_update(e, p, 16)                          # neither a state nor a (decay, t) pair
    with pytest.raises(RuntimeError):
        C.ema_update(e, p.double(), 16, decay=0.9, t=1)
    with pytest.raises(ValueError):
        C.arena_swap(e, e[4:], 8)                       # overlapping
    with pytest.raises(ValueError):
        C.arena_swap(e, p, 0)
    torch.cuda.synchronize()
    assert not e.any() and not p.any()


# ---------------------------------------------------------------- every training-step form
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture()
def nccl_world():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist.group.WORLD
    dist.destroy_process_group()


_data_cache = {}


def _data(rows, D, seed=7):
    key = (rows, D, seed)
    if key not in _data_cache:
        _data_cache.clear()
        X = torch.rand(rows, D, generator=torch.Generator().manual_seed(seed)).to(_dev())
        _data_cache[key] = (X, torch.arange(rows, device=_dev(), dtype=torch.int32))
    return _data_cache[key]


# form -> (kind, fused 28x28 step, reducer): the MLP with Adam fused into B3 and with e.adam() after a
# reducer; the conv layer path at 28x28 and 128x128; the fused 28x28 step; both comm-job tails (the fused
# xGMI reducer of one rank on the fused 28x28 step and on the layer path)
FORMS = {
    "mlp": ("mlp", None, None),
    "mlp_reducer": ("mlp", None, "rccl"),
    "conv28_fused": ("conv28", True, None),
    "conv28_layers": ("conv28", False, None),
    "conv128": ("conv128", False, None),
    "conv28_fused_comm": ("conv28", True, "xgmi"),
    "conv28_layers_comm": ("conv28", False, "xgmi"),
}
PLAIN = ("mlp", "conv28_fused", "conv28_layers", "conv128")


def _make(form, graphs=False, world=None, **kw):
    kind, f28, red = FORMS[form]
    kw.setdefault("lr", LR)
    if kind == "mlp":
        from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

        s = ck.SHAPES["tiny"]
        tr = MlpVaeTrainer(batch_size=s["B"], D=s["D"], H=s["H"], Z=s["Z"], device=_dev(), backend="hip", seed=3,
                           use_graphs=graphs, graph_steps=2, **kw)
        B, D = s["B"], s["D"]
    else:
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

        image = 28 if kind == "conv28" else 128
        B, D = 8, image * image
        tr = ConvVaeTrainer(batch_size=B, image=image, z=32 if image == 28 else 64, device=_dev(), backend="hip",
                            seed=2, use_graphs=graphs, graph_steps=2, **kw)
        if image == 28:
            assert tr.f28
            tr.f28 = f28
        assert tr.f28 == bool(f28)
    if red == "rccl":
        from multidisttorch_amd.parallel.ddp import make_arena_reducer

        tr.attach_reducer(make_arena_reducer(world, tr.grads, tr.bucket_bounds(None)))
    elif red == "xgmi":
        r = tr.C.XgmiP2PReducer(0, 1, tr.grads, tr.default_bucket_bounds(), True, 0.0, 64, 20.0, -1, True)
        assert r.fused()
        tr.attach_reducer(r)
    assert tr.use_graphs == graphs
    X, idx = _data(8 * B, D)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 4)
    return tr


def _train_state(tr, steps):
    torch.cuda.synchronize()
    st = tr.read_state()
    assert st["step"] == steps
    h = tr.loss_history()[:steps].copy()
    assert np.isfinite(h).all()
    return h, tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), st


def _same_training(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    for k, (x, y) in enumerate(zip(a[1:4], b[1:4])):
        assert torch.equal(x, y), ("params", "exp_avg", "exp_avg_sq")[k]
    assert a[4] == b[4], (a[4], b[4])


def _world(request, form):
    return request.getfixturevalue("nccl_world") if FORMS[form][2] == "rccl" else None


@pytest.mark.parametrize("form", list(FORMS))
def test_every_step_form_keeps_the_average(form, request, native_ext):
    """5 eager steps, the last a tail batch: training is bitwise that of the trainer without the average,
    the average follows the oracle step by step, and graph replay of the same steps ends bitwise there."""
    world = _world(request, form)
    a, b = _make(form, world=world, ema_decay=DECAY), _make(form, world=world)
    assert a.ema_on and a.ema.numel() == a.numel and torch.equal(a.ema, a.params) and not b.ema_on and b.ema is None
    e0 = a.ema.clone()
    ps, es = [], []
    for k in range(5):
        M = TAIL if k == 4 else None
        a.train_steps(1, M)
        b.train_steps(1, M)
        ps.append(a.params.clone())
        es.append(a.ema.clone())
    sa, sb = _train_state(a, 5), _train_state(b, 5)
    _same_training(sa, sb)
    assert not torch.equal(ps[-1], e0) and not torch.equal(es[-1], ps[-1])
    ec.check_chain(f"step {form}", e0, ps, es, DECAY)
    g = _make(form, graphs=True, world=world, ema_decay=DECAY)
    g.train_steps(4)
    g.train_steps(1, TAIL)
    _same_training(_train_state(g, 5), sa)
    assert torch.equal(g.ema, a.ema), float((g.ema - a.ema).abs().max())
    for tr in (a, b, g):
        tr.attach_reducer(None)


@pytest.mark.parametrize("form", PLAIN)
def test_no_learning_rate_no_movement(form, native_ext):
    tr = _make(form, ema_decay=0.999, lr=0.0)
    p0 = tr.params.clone()
    tr.train_steps(2)
    tr.train_steps(1, TAIL)
    torch.cuda.synchronize()
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, p0)


@pytest.mark.parametrize("form", ["mlp", "conv28_fused"])
def test_graph_picks_up_a_new_decay(form, native_ext):
    """The ramp (1 + t) / (10 + t) is below 0.9 for these steps, so a decay of 0.05 and then 0.2 is what matters."""
    g, e = _make(form, graphs=True, ema_decay=DECAY), _make(form, ema_decay=DECAY)
    for tr in (g, e):
        tr.train_steps(2)
        tr.set_hparams(ema_decay=0.05)
        tr.train_steps(2)
        tr.set_hparams(ema_decay=0.2)
        tr.train_steps(2)
    assert len(g._graphs) == 1  # one capture served all three values
    _same_training(_train_state(g, 6), _train_state(e, 6))
    assert torch.equal(g.ema, e.ema)
    k = _make(form, graphs=True, ema_decay=DECAY)   # each change mattered
    k.train_steps(6)
    _same_training(_train_state(k, 6), _train_state(g, 6))
    assert not torch.equal(k.ema, g.ema)
    # and the eager run followed the definition under the values in force
    o = _make(form, ema_decay=DECAY)
    prev = o.ema.clone()
    for t, d in enumerate((DECAY, DECAY, 0.05, 0.05, 0.2, 0.2), start=1):
        o.set_hparams(ema_decay=d)
        o.train_steps(1)
        e64, b = ec.bound(prev, o.params, d, t)
        ec.check(f"decay {d} at step {t} ({form})", o.ema, e64, b)
        prev = o.ema.clone()
    assert torch.equal(o.ema, e.ema)
    with pytest.raises(ValueError):
        _make(form).set_hparams(ema_decay=0.5)   # built without the launch


# ---------------------------------------------------------------- averaged_weights()
def _derived(tr):
    """The compute copies a conv trainer derives from its parameters."""
    return (tr.w16.clone(), tr.w16t.clone()) if hasattr(tr, "w16") else ()


@pytest.mark.parametrize("form", PLAIN)
def test_averaged_weights_context(form, native_ext):
    tr = _make(form, graphs=True, ema_decay=DECAY)
    tr.train_steps(4)
    X, idx = tr._data[0], tr._data[1][: tr.B + 5]
    z = torch.randn(3, tr.Z, generator=torch.Generator().manual_seed(1)).to(_dev())
    raw = tr.evaluate(X, idx)[0]        # captures the eval graphs and writes the transposed copies
    tr.evaluate_iw(X, idx, 4)
    tr.evaluate_latent(X, idx)
    torch.cuda.synchronize()
    p0, e0, d0 = tr.params.clone(), tr.ema.clone(), _derived(tr)
    ptrs = (tr.params.data_ptr(), tr.ema.data_ptr())
    with tr.averaged_weights():
        assert torch.equal(tr.params, e0) and torch.equal(tr.ema, p0)
        got = (tr.evaluate(X, idx), tr.evaluate_iw(X, idx, 4), tr.evaluate_latent(X, idx), tr.decode(z).clone())
        with pytest.raises(RuntimeError, match="does not nest"):
            with tr.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match="inside averaged_weights"):
            tr.train_steps(1)
    torch.cuda.synchronize()
    assert (tr.params.data_ptr(), tr.ema.data_ptr()) == ptrs
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, e0)
    for x, y in zip(_derived(tr), d0):
        assert torch.equal(x, y), "w16 / w16t changed across the context"
    # a fresh trainer that holds the average as its weights, at the same eval states
    ref = _make(form, graphs=True)
    ref.load_state_dict(tr.ema_state_dict())
    assert torch.equal(ref.params, e0)
    ref.evaluate(X, idx)
    ref.evaluate_iw(X, idx, 4)
    ref.evaluate_latent(X, idx)
    want = (ref.evaluate(X, idx), ref.evaluate_iw(X, idx, 4), ref.evaluate_latent(X, idx), ref.decode(z))
    assert got[0][0] == want[0][0] and torch.equal(got[0][1], want[0][1]) and got[0][0] != raw
    assert got[1] == want[1], (got[1], want[1])
    for k, v in want[2].items():
        assert torch.equal(got[2][k], v) if torch.is_tensor(v) else got[2][k] == v, k
    assert torch.equal(got[3], want[3])
    # 3 more steps: bitwise a run that never entered
    other = _make(form, graphs=True, ema_decay=DECAY)
    other.train_steps(4)
    tr.train_steps(2)
    tr.train_steps(1, TAIL)
    other.train_steps(2)
    other.train_steps(1, TAIL)
    _same_training(_train_state(tr, 7), _train_state(other, 7))
    assert torch.equal(tr.ema, other.ema)
    plain = _make(form)                 # no average: the context does nothing
    q = plain.params.clone()
    with plain.averaged_weights():
        plain.train_steps(1)
    assert not torch.equal(plain.params, q)


# ---------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("form", ["mlp", "conv28_fused"])
def test_checkpoint_round_trip_continues_bitwise(form, tmp_path, native_ext):
    from multidisttorch_amd.ckpt import checkpoint as ckpt
    from multidisttorch_amd.hpo.trial import build_specs

    spec = build_specs(1, 2, ema_decay=DECAY)[0]
    a = _make(form, ema_decay=DECAY)
    a.train_steps(3)
    ckpt.save_trial(str(tmp_path / "ck"), a, spec, 1)
    b = _make(form, ema_decay=DECAY)
    prog = ckpt.load_latest(str(tmp_path / "ck"), 0, b)
    assert prog["ema_decay"] == DECAY and torch.equal(b.ema, a.ema) and not torch.equal(b.ema, b.params)
    b.set_cursor(3, 4)
    straight = _make(form, ema_decay=DECAY)
    straight.train_steps(5)
    straight.train_steps(1, TAIL)
    b.train_steps(2)
    b.train_steps(1, TAIL)
    sb, ss = _train_state(b, 6), _train_state(straight, 6)
    for k, (x, y) in enumerate(zip(sb[1:4], ss[1:4])):
        assert torch.equal(x, y), k
    assert torch.equal(b.ema, straight.ema)
    # a checkpoint without an average: e = p
    plain = _make(form)
    plain.train_steps(3)
    ckpt.save_trial(str(tmp_path / "ck0"), plain, build_specs(1, 2)[0], 1)
    c = _make(form, ema_decay=DECAY)
    c.train_steps(1)
    prog0 = ckpt.load_latest(str(tmp_path / "ck0"), 0, c)
    torch.cuda.synchronize()
    assert prog0["ema_decay"] == 0.0 and torch.equal(c.ema, c.params) and torch.equal(c.params, plain.params)


# ---------------------------------------------------------------- two replicas sharing the GPU
def test_two_replicas_hold_bitwise_equal_averages():
    """Fresh processes (tests/gpu/ema_ddp_worker.py), each confined to its own CU share: the fused xGMI
    reducer's comm-job tail is followed by ``ema_update`` on every rank and the averages agree bitwise."""
    from multidisttorch_amd.launch import launch

    env = {"PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2", "MDT_CU_SPLIT": "1"}
    rc, outs = launch([sys.executable, os.path.join(HERE, "ema_ddp_worker.py"), str(DECAY)], 2, emulate="torchrun",
                      timeout=120, extra_env=env, capture=True)
    text = "\n".join(o or "" for o in outs)
    assert rc == 0, text[-4000:]
    res = {r["rank"]: r for r in (json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT "))}
    assert sorted(res) == [0, 1], text[-4000:]
    for r in res.values():
        assert r["reducer"] == "XgmiP2PReducer" and r["fused"] and r["status"] == 0, r
        assert r["tail"] == ["launch_jobs_multi", "ema_update"], r   # the comm-job tail, then the average
        assert r["params_equal"] and r["ema_equal"] and r["moved"] and r["finite"] and r["step"] == 6, r
    assert res[0]["losses"] != res[1]["losses"]   # the replicas drew their own noise


def test_worst_ratio_of_this_module():
    w = ec.worst()
    print(f"ema: worst error/bound of this run {w['ratio']:.3f} ({w['what']})")
    assert w["ratio"] <= 1.0
