"""The total-correlation penalty on the CPU: the oracle and its closed-form
gradient (models/tc.py against models/latent.py), the parsing of ``tc_weight``
into trial specs, the trial state's fields, and the torch backend of both
trainers."""
import math

import numpy as np
import pytest
import torch

from multidisttorch_amd.hpo.schedule import Schedule
from multidisttorch_amd.hpo.trial import TrialSpec, build_specs
from multidisttorch_amd.models import latent, tc
from multidisttorch_amd.ops import native
from multidisttorch_amd.ops.philox import reparam_eps
from tests import latent_cases as lc
from tests import tc_cases as tcc

needs_native = pytest.mark.skipif(not native.available(), reason="native extension not built")


# ---------------------------------------------------------------- oracle and gradient
@pytest.mark.parametrize("name,make", [("overlap", lc.overlap), ("mixed", lambda: lc.mixed(37, 12)),
                                       ("sharp", lambda: lc.sharp(37, 12))])
def test_value_and_closed_form_gradient(name, make):
    mulv = make()
    M, Z = mulv.shape[0], mulv.shape[1] // 2
    eps = tcc.noise(M, Z)
    v64, g64 = tcc.oracle(mulv, eps)
    m = mulv.double()
    rep = latent.latent_report(m[:, :Z], m[:, Z:], eps.double())
    assert abs(v64 - M * rep["tc"]) <= 1e-12 * max(1.0, abs(v64))
    val, am, al = tc.tc_closed_form(m[:, :Z], m[:, Z:], eps.double())
    assert abs(float(val) - v64) <= 1e-11 * max(1.0, abs(v64))
    err = float((torch.cat([am, al], 1) - g64).abs().max())
    print(f"{name}: tc_batch {v64:.6g}, max|g| {float(g64.abs().max()):.4g}, closed form vs autograd {err:.3g}")
    assert err <= 1e-12 * max(1.0, float(g64.abs().max()))
    # the float32 oracle stays finite (sharp: joint log-densities beyond +88.7)
    v32, g32 = tcc.oracle(mulv, eps, torch.float32)
    assert math.isfinite(v32) and torch.isfinite(g32).all()


def test_one_row_is_exactly_zero():
    mulv = lc.mixed(1, 12)
    eps = tcc.noise(1, 12)
    for dtype in (torch.float64, torch.float32):
        v, g = tcc.oracle(mulv, eps, dtype)
        assert v == 0.0 and not g.any()
        m = mulv.to(dtype)
        val, am, al = tc.tc_closed_form(m[:, :12], m[:, 12:], eps.to(dtype))
        assert float(val) == 0.0 and not am.any() and not al.any()


# ---------------------------------------------------------------- parsing and specs
def test_build_specs_takes_a_scalar_and_a_list():
    assert [s.tc_weight for s in build_specs(3, 1)] == [0.0, 0.0, 0.0]
    assert [s.tc_weight for s in build_specs(3, 1, tc_weight=2)] == [2.0, 2.0, 2.0]
    assert [s.tc_weight for s in build_specs(3, 1, tc_weight="0,1.5")] == [0.0, 1.5, 0.0]
    assert [s.tc_weight for s in build_specs(2, 1, tc_weight=[0.5, 3])] == [0.5, 3.0]
    assert build_specs(2, 1, tc_weight="0,7")[1].to_dict()["tc_weight"] == 7.0
    assert TrialSpec(0, 1, 1e-3, 1.0, 0).to_dict()["tc_weight"] == 0.0


@pytest.mark.parametrize("bad", [-1, "-0.5", "1,nan", float("inf"), "inf", [0.0, float("nan")]])
def test_build_specs_rejects_bad_weights(bad):
    with pytest.raises(ValueError, match="tc_weight must be finite and >= 0"):
        build_specs(2, 1, tc_weight=bad)


# ---------------------------------------------------------------- trial state
@needs_native
def test_state_carries_the_weight_and_the_running_sum():
    C = native.require()
    s = C.TrialState(-1)
    s.set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 3, False, kl_anneal_steps=4, tc_weight=2.0)
    assert len(s.read_state(False)) == 8
    for t, want in ((0, 0.0), (1, 0.5), (3, 1.5), (4, 2.0), (9, 2.0)):
        s.set_step(False, t)
        s.set_step(True, t)
        assert s.read_tc(False) == [want, 0.0] and s.read_tc(True) == [0.0, 0.0]
    with pytest.raises(ValueError, match="tc_weight"):
        s.set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 3, False, tc_weight=-1.0)


# ---------------------------------------------------------------- torch-backend trainers
def _data(D=784, rows=64):
    X = torch.rand(rows, D, generator=torch.Generator().manual_seed(0))
    return X, torch.arange(rows, dtype=torch.int32)


def _mlp(**kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    return MlpVaeTrainer(batch_size=16, D=64, H=32, Z=8, device="cpu", backend="torch", seed=1, **kw), 64


def _conv(**kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    return ConvVaeTrainer(batch_size=8, image=28, z=8, device="cpu", backend="torch", seed=1, **kw), 784


def _run(make, steps=3, **kw):
    tr, D = make(**kw)
    X, idx = _data(D)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 4)
    tr.train_steps(steps)
    return tr


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_zero_weight_is_the_trainer_without_the_argument(make):
    a, b = _run(make), _run(make, tc_weight=0.0)
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg)
    np.testing.assert_array_equal(a.loss_history(), b.loss_history())
    assert b.read_state()["tc_weight"] == 0.0 and b.read_state()["epoch_tc"] == 0.0
    with pytest.raises(ValueError, match="built with tc_weight > 0"):
        b.set_hparams(tc_weight=1.0)
    with pytest.raises(ValueError, match="tc_weight must be finite"):
        make(tc_weight=float("nan"))


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_weight_follows_the_kl_anneal_and_epoch_tc_is_the_oracle_sum(make):
    tr, D = make(tc_weight=2.0, schedule=Schedule(kl_anneal_steps=4))
    ref, _ = make()
    X, idx = _data(D, 8 * tr.B)
    for t in (tr, ref):
        t.bind_train_data(X, idx)
        t.set_cursor(0, 8)
    want = 0.0
    for t in range(1, 7):
        # the oracle on the rows this step encodes, from the weights before the step
        rows = X[idx[(t - 1) * tr.B: t * tr.B].long()]
        eps = torch.from_numpy(reparam_eps(tr.B, tr.Z, tr.seed, tr.rng_stream, t - 1))
        with torch.no_grad():
            mu, lv = tr._lat_encode_torch(rows)
        want += tcc.oracle(torch.cat([mu, lv], 1), eps)[0]
        tr.train_steps(1)
        st = tr.read_state()
        assert st["tc_weight"] == 2.0 * min(t / 4.0, 1.0) and st["step"] == t
        assert abs(st["epoch_tc"] - want) <= 1e-4 * max(1.0, abs(want)), (t, st["epoch_tc"], want)
    ref.set_schedule(Schedule(kl_anneal_steps=4))
    ref.train_steps(6)
    assert not torch.equal(ref.params, tr.params)                      # the penalty entered the gradients
    # the ring keeps meaning BCE + kl_t * KL (the MLP reference may run the fused native CPU step: rounding)
    assert abs(tr.loss_history()[0] - ref.loss_history()[0]) <= 1e-5 * abs(ref.loss_history()[0])
    tr.reset_loss()
    assert tr.read_state()["epoch_tc"] == 0.0
    assert tr.read_state(eval=True)["tc_weight"] == 0.0
    tr.set_hparams(tc_weight=0.0)                                      # down to 0 is allowed, and back up
    tr.set_hparams(tc_weight=1.0)
    assert tr.read_state()["tc_weight"] == 1.0


@needs_native
def test_mlp_cpu_trainer_leaves_the_native_step_for_the_penalty():
    a, _ = _mlp()
    b, _ = _mlp(tc_weight=1.0)
    assert a._cpu_native() is not None and b._cpu_native() is None
