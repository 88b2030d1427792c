"""Weight averaging (``ema_decay``) without a GPU: the torch backends of both
trainers (the native CPU MLP step included) against the float64 oracle of
tests/ema_cases.py, the ``averaged_weights()`` context, the domain of the decay,
per-trial parsing, the ``TrialSpec`` round trip and the checkpoint fields."""
import math

import pytest
import torch

from multidisttorch_amd.ckpt import checkpoint as ckpt
from multidisttorch_amd.hpo import runner
from multidisttorch_amd.hpo.trial import TrialSpec, build_specs
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from multidisttorch_amd.models.trainer_base import check_ema_decay, ema_omd
from tests import ema_cases as ec

DECAY = 0.9


def _mlp(**kw):
    kw.setdefault("lr", 3e-3)
    tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", seed=3, **kw)
    X = torch.rand(64, 20, generator=torch.Generator().manual_seed(7))
    tr.bind_train_data(X, torch.arange(64, dtype=torch.int32))
    tr.set_cursor(0, 4)
    return tr


def _conv(**kw):
    kw.setdefault("lr", 3e-3)
    tr = ConvVaeTrainer(batch_size=8, image=28, z=32, backend="torch", device="cpu", seed=2, **kw)
    X = torch.rand(32, 784, generator=torch.Generator().manual_seed(7))
    tr.bind_train_data(X, torch.arange(32, dtype=torch.int32))
    tr.set_cursor(0, 4)
    return tr


MAKERS = {"mlp": _mlp, "conv28": _conv}


def _stock(monkeypatch):
    monkeypatch.setattr(MlpVaeTrainer, "_cpu_native", lambda self: None)


# ---------------------------------------------------------------- the rule
def test_domain_of_the_decay():
    assert check_ema_decay(0) == 0.0 and check_ema_decay("0.999") == 0.999
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="ema_decay must be in"):
            check_ema_decay(bad)
        with pytest.raises(ValueError, match="ema_decay must be in"):
            _mlp(ema_decay=bad)
    tr = _mlp()
    assert not tr.ema_on and tr.ema is None
    tr.set_hparams(ema_decay=0.0)
    with pytest.raises(ValueError, match="built with ema_decay > 0"):
        tr.set_hparams(ema_decay=0.5)
    with pytest.raises(ValueError):
        _mlp(ema_decay=0.5).set_hparams(ema_decay=1.0)


def test_the_ramp_meets_the_decay_where_the_definition_says():
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    for t in (1, 5, 79):
        assert ema_omd(0.9, t) == f32(1.0 - (1.0 + t) / (10.0 + t))   # the ramp is below the decay
    assert ec.d_t(0.9, 80) == 0.9 == (1.0 + 80) / (10.0 + 80)          # they meet at t = 80
    for t in (80, 81, 10 ** 6):
        assert ema_omd(0.9, t) == f32(1.0 - 0.9)
    assert ema_omd(0.999, 10 ** 6) == f32(1.0 - 0.999) and ema_omd(0.999, 81) == f32(1.0 - 82.0 / 91.0)
    assert ema_omd(0.0, 7) == 1.0


def test_native_binding_forms_the_same_factor(native_ext):
    from multidisttorch_amd.ops import native

    C = native.require()
    for decay in ec.DECAYS + (0.0, 0.5):
        for t in ec.TS + (2, 9, 8990, 8991):
            assert C.ema_omd(decay, t) == ema_omd(decay, t), (decay, t)


# ---------------------------------------------------------------- torch-backend steps
@pytest.mark.parametrize("form", ["mlp_native", "mlp_stock", "conv28"])
def test_torch_steps_match_the_oracle_and_leave_training_alone(form, monkeypatch, native_ext):
    if form == "mlp_stock":
        _stock(monkeypatch)
    make = MAKERS["conv28" if form == "conv28" else "mlp"]
    a, b = make(ema_decay=DECAY), make()
    if form == "mlp_native":
        assert a._cpu_native() is not None
    assert a.ema_on and torch.equal(a.ema, a.params) and a.ema.data_ptr() != a.params.data_ptr()
    e0 = a.ema.clone()
    ps, es = [], []
    for k in range(5):
        M = 5 if k == 4 else None   # a tail batch last
        a.train_steps(1, M)
        b.train_steps(1, M)
        ps.append(a.params.clone())
        es.append(a.ema.clone())
    for n in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert (a.loss_history() == b.loss_history()).all() and a.read_state() == b.read_state()
    ec.check_chain(f"torch {form}", e0, ps, es, DECAY)
    assert not torch.equal(a.ema, a.params)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_no_learning_rate_no_movement(kind, native_ext):
    tr = MAKERS[kind](ema_decay=0.999, lr=0.0)
    p0 = tr.params.clone()
    tr.train_steps(3)
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, p0)   # e == p is a bitwise fixed point


def test_a_changed_decay_is_used_by_the_next_step(native_ext):
    a, b = _mlp(ema_decay=0.5), _mlp(ema_decay=0.5)
    a.train_steps(3)
    b.train_steps(3)
    a.set_hparams(ema_decay=0.05)
    e_prev = a.ema.clone()
    a.train_steps(1)
    b.train_steps(1)
    e64, bd = ec.bound(e_prev, a.params, 0.05, 4)
    ec.check("torch mlp after set_hparams", a.ema, e64, bd)
    assert torch.equal(a.params, b.params) and not torch.equal(a.ema, b.ema)


# ---------------------------------------------------------------- averaged_weights()
@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_averaged_weights_context(kind, native_ext):
    make = MAKERS[kind]
    tr = make(ema_decay=DECAY)
    tr.train_steps(4)
    X, idx = tr._data[0], tr._data[1][:21]
    p0, e0 = tr.params.clone(), tr.ema.clone()
    z = torch.randn(3, tr.Z, generator=torch.Generator().manual_seed(1))
    raw = tr.evaluate(X, idx)[0]
    with tr.averaged_weights() as inner:
        assert inner is tr and torch.equal(tr.params, e0) and torch.equal(tr.ema, p0)
        got = (tr.evaluate(X, idx), tr.evaluate_iw(X, idx, 4), tr.evaluate_latent(X, idx), tr.decode(z))
        with pytest.raises(RuntimeError, match="does not nest"):
            with tr.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match="inside averaged_weights"):
            tr.train_steps(1)
        with pytest.raises(RuntimeError, match="inside averaged_weights"):
            tr.optimizer_state()
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, e0)
    # a fresh trainer that holds the average as its weights, at the same eval state
    ref = make()
    ref.load_state_dict(tr.ema_state_dict())
    assert torch.equal(ref.params, e0)
    ref.evaluate(X, idx)   # tr's raw pass above: the eval noise follows the eval state's step
    want = (ref.evaluate(X, idx), ref.evaluate_iw(X, idx, 4), ref.evaluate_latent(X, idx), ref.decode(z))
    assert got[0][0] == want[0][0] and torch.equal(got[0][1], want[0][1]) and got[0][0] != raw
    assert got[1] == want[1]
    for k, v in want[2].items():
        assert torch.equal(got[2][k], v) if torch.is_tensor(v) else got[2][k] == v, k
    assert torch.equal(got[3], want[3])
    # training goes on as if the context had never been entered
    other = make(ema_decay=DECAY)
    other.train_steps(4)
    other.evaluate(X, idx)
    tr.train_steps(3)
    other.train_steps(3)
    assert torch.equal(tr.params, other.params) and torch.equal(tr.ema, other.ema)
    # without an average the context changes nothing
    plain = make()
    q = plain.params.clone()
    with plain.averaged_weights():
        assert torch.equal(plain.params, q)
        plain.train_steps(1)
    with pytest.raises(ValueError):
        plain.load_ema_state_dict(tr.ema_state_dict())
    assert all(torch.equal(v, plain.state_dict()[k]) for k, v in plain.ema_state_dict().items())


def test_state_dicts_use_the_parameter_names(native_ext):
    tr = _mlp(ema_decay=DECAY)
    tr.train_steps(2)
    sd = tr.ema_state_dict()
    assert list(sd) == list(tr.state_dict()) and "fc1.weight" in sd
    assert any(not torch.equal(sd[k], tr.state_dict()[k]) for k in sd)
    other = _mlp(ema_decay=DECAY)
    other.load_ema_state_dict(sd)
    assert torch.equal(other.ema, tr.ema)
    other.load_state_dict(tr.state_dict())     # parameters set from outside a step: e = p
    assert torch.equal(other.ema, other.params) and torch.equal(other.params, tr.params)


# ---------------------------------------------------------------- CLI values, trial specs
def test_per_trial_parsing_and_round_trip():
    specs = build_specs(3, 1, ema_decay="0,0.99")
    assert [s.ema_decay for s in specs] == [0.0, 0.99, 0.0]
    assert [s.ema_decay for s in build_specs(2, 1, ema_decay=0.5)] == [0.5, 0.5]
    assert [s.ema_decay for s in build_specs(2, 1, ema_decay=[0.1, 0.2])] == [0.1, 0.2]
    assert [s.ema_decay for s in build_specs(2, 1)] == [0.0, 0.0]
    for bad in ("0.5,1", "-0.1", "nan", "inf", 1.0):
        with pytest.raises(ValueError, match="ema_decay must be"):
            build_specs(2, 1, ema_decay=bad)
    d = specs[1].to_dict()
    assert d["ema_decay"] == 0.99 and TrialSpec(**d) == specs[1]
    assert TrialSpec(0, 1, 1e-3, 1.0, 0).ema_decay == 0.0


# ---------------------------------------------------------------- checkpoints
def test_checkpoint_fields_resume_and_the_refused_resume(tmp_path, native_ext):
    spec = build_specs(1, 2, ema_decay=DECAY)[0]
    a = _mlp(ema_decay=DECAY)
    a.train_steps(3)
    path = ckpt.save_trial(str(tmp_path / "ck"), a, spec, 1)
    ck = torch.load(path, weights_only=True)
    assert ck["objective"]["ema_decay"] == DECAY and ck["trial"]["ema_decay"] == DECAY
    assert torch.equal(ck["optimizer"]["ema"], a.ema) and not torch.equal(ck["optimizer"]["ema"], a.params)
    # save, load into a fresh trainer, continue: a straight run
    b = _mlp(ema_decay=DECAY)
    prog = ckpt.load_latest(str(tmp_path / "ck"), 0, b)
    assert prog["ema_decay"] == DECAY and torch.equal(b.ema, a.ema) and torch.equal(b.params, a.params)
    b.set_cursor(3, 4)
    straight = _mlp(ema_decay=DECAY)
    straight.train_steps(6)
    b.train_steps(3)
    assert torch.equal(b.params, straight.params) and torch.equal(b.ema, straight.ema)
    # the runner refuses another value
    runner._check_resumed(prog, spec, runner.RunOptions())
    runner._check_resumed(None, spec, runner.RunOptions())
    other = build_specs(1, 2, ema_decay=0.99)[0]
    with pytest.raises(ValueError, match=r"was trained with --ema-decay 0\.9, this run asks for --ema-decay 0\.99"):
        runner._check_resumed(prog, other, runner.RunOptions())
    # a checkpoint of a run without averaging: no fields, loads as 0, and an averaging trainer starts at e = p
    plain = _mlp()
    plain.train_steps(3)
    spec0 = build_specs(1, 2)[0]
    path0 = ckpt.save_trial(str(tmp_path / "ck0"), plain, spec0, 1)
    ck0 = torch.load(path0, weights_only=True)
    assert "ema" not in ck0["optimizer"] and "ema_decay" not in ck0["objective"]
    c = _mlp(ema_decay=DECAY)
    c.train_steps(1)
    prog0 = ckpt.load_latest(str(tmp_path / "ck0"), 0, c)
    assert prog0["ema_decay"] == 0.0 and torch.equal(c.ema, c.params) and torch.equal(c.params, plain.params)
    with pytest.raises(ValueError, match="was trained with --ema-decay 0.0"):
        runner._check_resumed(prog0, spec, runner.RunOptions())
    assert math.isfinite(float(c.ema.abs().sum()))
