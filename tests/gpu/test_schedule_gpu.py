"""Device-resident lr / KL-weight schedules (hpo/schedule.py) on the HIP backend.

The oracle throughout: a second trainer WITHOUT a schedule, run eagerly, whose
host sets ``lr * f_lr(t)`` and ``kl_beta * f_kl(t)`` before each step t. Both
trainers run the same kernels on the same inputs, and for warm-up and annealing
``t / W`` and the products are the same IEEE operations on both sides, so the
results are bitwise equal: parameters, both Adam moments, the loss ring and the
read-back effective ``lr`` / ``kl_beta``. Cosine decay goes through the
device's ``cospi``: its read-back lr is held to the Python formula at 1e-12
and the parameters to the project's Adam tolerance.
"""

import pytest
import torch

from multidisttorch_amd.hpo.schedule import Schedule

pytestmark = pytest.mark.gpu

LR, BETA = 2e-3, 2.0
WARM = Schedule(lr_warmup_steps=3, kl_anneal_steps=5)
COS = Schedule(lr_warmup_steps=2, lr_decay="cosine", lr_decay_steps=8, lr_min_ratio=0.1)


def _data(rows, D, seed=1):
    dev = torch.device("cuda")
    X = torch.rand(rows, D, generator=torch.Generator().manual_seed(seed)).to(dev)
    return X, torch.arange(rows, device=dev, dtype=torch.int32)


def _conv(X, idx, B, schedule=None, graphs=False, **kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=B, device=torch.device("cuda"), backend="hip", seed=3, lr=LR, kl_beta=BETA,
                        use_graphs=graphs, graph_steps=4, schedule=schedule, **kw)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 8)
    return tr


def _mlp(X, idx, B=32, schedule=None, graphs=False, **kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    tr = MlpVaeTrainer(batch_size=B, device=torch.device("cuda"), backend="hip", seed=3, lr=LR, kl_beta=BETA,
                       use_graphs=graphs, graph_steps=4, schedule=schedule, **kw)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 8)
    return tr


def _oracle_step(o, s, t, M=None):
    """Step t of the host-driven oracle: the effective values pushed from the host."""
    o.set_hparams(lr=LR * s.lr_factor(t), kl_beta=BETA * s.kl_factor(t))
    o.train_steps(1, M)


def _same(a, b, steps):
    torch.cuda.synchronize()
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    ha, hb = a.loss_history()[:steps], b.loss_history()[:steps]
    assert (ha == hb).all() and (ha == ha).all(), (ha, hb)
    sa, sb = a.read_state(), b.read_state()
    assert sa == sb and sa["step"] == steps, (sa, sb)


def _three_way(make, s, steps, tail_M):
    """Device schedule under graphs (4-step graph replayed: a different t at
    every step inside it, crossing W and A inside a replay), device schedule
    eager, and the host-driven oracle; then one eager tail step of tail_M rows."""
    g, e, o = make(schedule=s, graphs=True), make(schedule=s), make()
    g.train_steps(steps)
    for t in range(1, steps + 1):
        e.train_steps(1)
        _oracle_step(o, s, t)
        se, so = e.read_state(), o.read_state()  # what the kernels of step t used
        assert se["lr"] == so["lr"] == LR * s.lr_factor(t), (t, se, so)
        assert se["kl_beta"] == so["kl_beta"] == float(torch.tensor(BETA * s.kl_factor(t), dtype=torch.float32))
    _same(g, o, steps)
    _same(e, o, steps)
    g.use_graphs = False
    g.train_steps(1, tail_M)
    e.train_steps(1, tail_M)
    _oracle_step(o, s, steps + 1, tail_M)
    _same(g, o, steps + 1)
    _same(e, o, steps + 1)
    return g, e, o


def test_fused28_warmup_anneal_bitwise(native_ext):
    """The fused 28x28 step (its forward/backward run before the step is
    advanced and use t = step + 1)."""
    X, idx = _data(256, 784)
    trs = _three_way(lambda **kw: _conv(X, idx, 32, **kw), WARM, 12, 13)
    for tr in trs:
        assert tr.f28
        assert int(tr.f28_err.item()) == 0


def test_layer_path28_warmup_anneal_bitwise(native_ext, monkeypatch):
    monkeypatch.setenv("MDT_CONV_F28", "0")
    X, idx = _data(256, 784)
    trs = _three_way(lambda **kw: _conv(X, idx, 16, **kw), WARM, 12, 13)
    assert not any(tr.f28 for tr in trs)


def test_layer_path128_warmup_anneal_bitwise(native_ext):
    """128x128: the first layer's thin kernels hold two of the step-advance sites."""
    X, idx = _data(64, 128 * 128)
    _three_way(lambda **kw: _conv(X, idx, 8, image=128, z=64, **kw), WARM, 6, 5)


def test_mlp_fused_adam_warmup_anneal_bitwise(native_ext):
    """Adam in the B3 epilogues, decoupled weight decay on ((float)lr_t scales it)."""
    X, idx = _data(256, 784)
    _three_way(lambda **kw: _mlp(X, idx, weight_decay=0.01, decoupled_wd=True, **kw), WARM, 12, 13)


def test_mlp_unfused_adam_warmup_anneal_bitwise(native_ext):
    """forward / backward(fuse_adam=False) / adam(): the step as it runs with a
    reducer attached, through the streaming Adam kernel (adam_flat)."""
    X, idx = _data(256, 784)
    a = _mlp(X, idx, schedule=WARM, weight_decay=0.01, decoupled_wd=True)
    o = _mlp(X, idx, weight_decay=0.01, decoupled_wd=True)

    def step(tr):
        tr.engine.forward(X, tr._data[1], 32, True, False, tr.rng_stream, False)
        tr.engine.backward(X, tr._data[1], 32, 0, False)
        tr.engine.adam()

    for t in range(1, 5):
        o.set_hparams(lr=LR * WARM.lr_factor(t), kl_beta=BETA * WARM.kl_factor(t))
        step(a)
        step(o)
        _same(a, o, t)
        assert a.read_state()["lr"] == LR * WARM.lr_factor(t)


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_cosine_lr_matches_formula(native_ext, kind):
    """Cosine decay: the device's cospi may differ from the host's cos in the
    last ulps, so instead of bitwise: the read-back lr of every step against
    the Python formula at rel 1e-12 (double cos is good to a few ulp on a
    factor >= 0.1), and the parameters after each step against the oracle
    re-synced from the device trainer, at the project's Adam tolerance
    (test_f28_adam_matches_torch_optim: rtol 1e-5, atol 1e-7)."""
    X, idx = _data(256, 784)
    make = (lambda **kw: _conv(X, idx, 32, **kw)) if kind == "conv28" else (lambda **kw: _mlp(X, idx, **kw))
    a, o = make(schedule=COS), make()
    for t in range(1, 9):
        for name in ("params", "exp_avg", "exp_avg_sq"):
            getattr(o, name).copy_(getattr(a, name))
        o.refresh_weights()
        o.set_step(t - 1)
        o.set_cursor((t - 1) % 8, 8)
        _oracle_step(o, COS, t)
        a.train_steps(1)
        torch.cuda.synchronize()
        want = LR * COS.lr_factor(t)
        got = a.read_state()["lr"]
        assert abs(got - want) <= 1e-12 * want, (t, got, want)
        torch.testing.assert_close(a.params, o.params, rtol=1e-5, atol=1e-7)
    assert a.read_state()["lr"] < 0.11 * LR  # the floor r = 0.1 at t = T


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_eval_uses_full_beta(native_ext, kind):
    """Annealing barely started (A = 1000, 12 steps), yet evaluate() returns
    bitwise the total of a schedule-free trainer holding the same weights."""
    X, idx = _data(256, 784)
    make = (lambda **kw: _conv(X, idx, 32, **kw)) if kind == "conv28" else (lambda **kw: _mlp(X, idx, **kw))
    a, b = make(schedule=Schedule(kl_anneal_steps=1000), graphs=True), make(graphs=True)
    a.train_steps(12)
    assert a.read_state()["kl_beta"] == float(torch.tensor(BETA * 12 / 1000, dtype=torch.float32))
    b.load_state_dict(a.state_dict())
    ev = idx[:64]
    la, _ = a.evaluate(X, ev, want_first_recon=False)
    lb, _ = b.evaluate(X, ev, want_first_recon=False)
    assert la == lb and la == la and la > 0
    assert a.read_state(eval=True)["kl_beta"] == BETA


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_zero_schedule_is_no_schedule(native_ext, kind):
    X, idx = _data(256, 784)
    make = (lambda **kw: _conv(X, idx, 32, **kw)) if kind == "conv28" else (lambda **kw: _mlp(X, idx, **kw))
    a, b = make(schedule=Schedule(), graphs=True), make(graphs=True)
    a.train_steps(6)
    b.train_steps(6)
    _same(a, b, 6)
    st = a.read_state()
    assert st["lr"] == LR and st["kl_beta"] == BETA
