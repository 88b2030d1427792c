"""The trial-state owner of both trainers (csrc/runtime/trial_state.h) on the
host: ``TrialState(-1)`` keeps its three buffers in host memory, so what
tests/gpu/test_schedule_gpu.py asserts of the read-back effective lr / KL
weight on the device is asserted here of the host side alone (set_step /
set_hparams re-seeding them and the beta^t products)."""
import struct

import numpy as np
import pytest

from multidisttorch_amd.hpo.schedule import Schedule
from multidisttorch_amd.ops import native

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")

LR, BETA = 2e-3, 2.0
WARM = Schedule(lr_warmup_steps=3, kl_anneal_steps=5)
COS = Schedule(lr_warmup_steps=2, lr_decay="cosine", lr_decay_steps=8, lr_min_ratio=0.1)
# byte offsets in TrainState (csrc/kernels/vae_mlp.h): b1pow, b2pow after step (8) and cursor, nbatches (4 + 4);
# the loss ring after epoch_loss, epoch_count, lr_t (8 each) and kl_t, kl_next, sched_off, pad_ (4 each)
B1POW, RING = 16, 72


def _state(schedule=None, b1=0.9, b2=0.999):
    s = native.require().TrialState(-1)
    assert s.train_state.device.type == s.eval_state.device.type == s.hparams.device.type == "cpu"
    _hparams(s, schedule, b1, b2)
    return s


def _hparams(s, schedule, b1=0.9, b2=0.999):
    s.set_hparams(LR, b1, b2, 1e-8, 0.0, BETA, 1.0, 3, False, **(schedule or Schedule()).native_args())


def _read(s, eval=False):
    return dict(zip(("step", "cursor", "nbatches", "epoch_loss", "epoch_count", "lr", "kl_beta"), s.read_state(eval)))


def _pows(s, eval=False):
    t = s.eval_state if eval else s.train_state
    return struct.unpack("<2d", bytes(t[B1POW:B1POW + 16].tolist()))


def _f32(v):
    return float(np.float32(v))


def test_warmup_anneal_effective_values_exact():
    s = _state(WARM)
    for t in (0, 1, WARM.lr_warmup_steps, WARM.lr_warmup_steps + 1):
        s.set_step(False, t)
        st = _read(s)
        assert st["step"] == t
        assert st["lr"] == LR * WARM.lr_factor(t), (t, st)
        assert st["kl_beta"] == _f32(BETA * WARM.kl_factor(t)), (t, st)


def test_cosine_lr_matches_formula():
    s = _state(COS)
    for t in range(1, 9):
        s.set_step(False, t)
        want, got = LR * COS.lr_factor(t), _read(s)["lr"]
        assert abs(got - want) <= 1e-12 * want, (t, got, want)
    assert _read(s)["lr"] < 0.11 * LR  # the floor r = 0.1 at t = T


def test_eval_state_reads_full_values():
    s = _state(WARM)
    for t in (0, 1, 4):
        s.set_step(False, t)
        s.set_step(True, t)
        st = _read(s, eval=True)
        assert st["step"] == t and st["lr"] == LR and st["kl_beta"] == BETA, (t, st)
    _hparams(s, Schedule(kl_anneal_steps=1000))
    st = _read(s, eval=True)
    assert st["lr"] == LR and st["kl_beta"] == BETA


def test_new_betas_reseed_the_products():
    s = _state()
    s.set_step(False, 7)
    assert _pows(s) == (0.9 ** 7, 0.999 ** 7)
    _hparams(s, None, 0.8, 0.95)
    assert _pows(s) == (0.8 ** 7, 0.95 ** 7)
    assert _pows(s, eval=True) == (1.0, 1.0)  # eval step 0
    assert _read(s)["step"] == 7


def test_cursor_loss_and_history_round_trip():
    C = native.require()
    s = _state()
    for ev in (False, True):
        s.set_cursor(ev, 5, 9)
        st = _read(s, ev)
        assert (st["cursor"], st["nbatches"]) == (5, 9)
        other = _read(s, not ev)
        assert (other["cursor"], other["nbatches"]) == ((5, 9) if ev else (0, 0))
        # epoch_loss, epoch_count: the two doubles after the beta^t products
        t = s.eval_state if ev else s.train_state
        t[B1POW + 16:B1POW + 32] = t.new_tensor(list(struct.pack("<2d", 12.5, 3.0)))
        st = _read(s, ev)
        assert (st["epoch_loss"], st["epoch_count"]) == (12.5, 3.0)
        s.reset_loss(ev)
        st = _read(s, ev)
        assert (st["epoch_loss"], st["epoch_count"], st["cursor"], st["nbatches"]) == (0.0, 0.0, 5, 9)
        h = s.loss_history(ev).numpy()
        assert h.shape == (C.kLossHist,) and h.dtype == np.float32 and not h.any()
        last = RING + 4 * (C.kLossHist - 1)
        assert last + 4 <= t.numel()
        t[last:last + 4] = t.new_tensor(list(struct.pack("<f", 1.5)))
        h = s.loss_history(ev).numpy()
        assert h[-1] == 1.5 and not h[:-1].any()
