"""The driver-facing contract both trainers inherit from ``VaeTrainerBase``
(models/trainer_base.py), on the torch backend: hyper-parameter keys, the eval
cursor, checkpoint round trips and the loss ring behave the same for the MLP
and the conv trainer because neither carries a copy of its own."""
import numpy as np
import pytest
import torch

from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from multidisttorch_amd.models.trainer_base import VaeTrainerBase

SHARED = ("read_state", "reset_loss", "loss_history", "set_hparams", "set_schedule", "_effective", "prepare",
          "_replay", "optimizer_state", "load_optimizer_state")


def _mlp(**kw):
    return MlpVaeTrainer(batch_size=8, D=16, H=8, Z=4, device="cpu", backend="torch", seed=3, **kw)


def _conv(**kw):
    return ConvVaeTrainer(batch_size=4, image=28, device="cpu", backend="torch", seed=3, **kw)


@pytest.fixture(params=["mlp", "conv"])
def make(request):
    return _mlp if request.param == "mlp" else _conv


def _bound(make, **kw):
    tr = make(**kw)
    n = 5 * tr.B
    X = torch.rand(n, tr.D, generator=torch.Generator().manual_seed(1))
    tr.bind_train_data(X, torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(torch.int32))
    tr.set_cursor(0, 5)
    return tr, X


def test_unknown_hparam_is_refused(make):
    tr = make()
    with pytest.raises(KeyError):
        tr.set_hparams(bogus=1)
    assert "bogus" not in tr.hp
    tr.set_hparams(lr=5e-4)
    assert tr.hp["lr"] == 5e-4


def test_eval_pass_wraps_the_cursor(make):
    tr, X = _bound(make)
    n = 2 * tr.B + tr.B // 2  # 2.5 batches
    total, first = tr.evaluate(X, torch.arange(n, dtype=torch.int32))
    st = tr.read_state(eval=True)
    assert (st["cursor"], st["step"], st["epoch_count"], st["nbatches"]) == (0, 3, 3, 3), st
    assert total == st["epoch_loss"] and total == total and total > 0
    assert first.shape == (tr.B, tr.D)
    assert tr.read_state()["step"] == 0  # the training state is not touched


def test_checkpoint_round_trip_is_exact(make):
    a, X = _bound(make, lr=2e-3, kl_beta=2.0)
    a.train_steps(3)
    b, _ = _bound(make, lr=2e-3, kl_beta=2.0)
    b.load_state_dict(a.state_dict())
    b.load_optimizer_state(a.optimizer_state())
    b.set_cursor(a.read_state()["cursor"], 5)
    assert b.step_count == a.step_count == 3
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    a.train_steps(1)
    b.train_steps(1)
    la, lb = a.loss_history()[3], b.loss_history()[3]
    assert la == lb and la == la
    assert torch.equal(a.params, b.params)


def test_loss_ring_holds_the_per_step_losses(make):
    tr, _ = _bound(make)
    losses = []
    for _ in range(6):  # wraps the 5-batch epoch once
        tr.reset_loss()
        tr.train_steps(1)
        st = tr.read_state()
        assert st["epoch_count"] == 1
        losses.append(st["epoch_loss"])
    assert st["step"] == 6 and st["cursor"] == 1
    hist = tr.loss_history()
    assert np.array_equal(hist[:6], np.asarray(losses, np.float32))
    assert not hist[6:].any()


@pytest.mark.parametrize("cls", [MlpVaeTrainer, ConvVaeTrainer])
def test_shared_methods_are_written_once(cls):
    assert issubclass(cls, VaeTrainerBase)
    again = [m for m in SHARED if m in cls.__dict__]
    assert not again, f"{cls.__name__} redefines {again}: they belong to VaeTrainerBase"
