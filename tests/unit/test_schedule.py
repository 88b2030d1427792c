"""lr / KL-weight schedules (hpo/schedule.py): the factor functions, their
validation, both trainers' torch backends against a host-driven oracle (a
schedule-free trainer whose host sets ``lr * f_lr(t)`` / ``kl_beta * f_kl(t)``
before each step: the same IEEE products, so bitwise), checkpoint resume, the
command line, and one run through the HPO runner on the CPU backend."""

import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from multidisttorch_amd.ckpt import checkpoint as ckpt
from multidisttorch_amd.hpo.schedule import Schedule
from multidisttorch_amd.hpo.trial import TrialSpec, build_specs
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LR, BETA = 2e-3, 2.0
FULL = Schedule(lr_warmup_steps=4, lr_decay="cosine", lr_decay_steps=12, lr_min_ratio=0.1, kl_anneal_steps=5)


def test_factor_table():
    s = FULL
    assert s.lr_factor(1) == 0.25 and s.lr_factor(4) == 1.0
    assert s.lr_factor(5) == 0.1 + 0.9 * 0.5 * (1.0 + math.cos(math.pi / 8))
    assert s.lr_factor(5) == pytest.approx(0.1 + 0.45 * (1 + math.cos(math.pi / 8)), rel=1e-15)
    assert s.lr_factor(12) == s.lr_factor(20) == pytest.approx(0.1, rel=1e-15)
    assert s.kl_factor(1) == 0.2 and s.kl_factor(5) == s.kl_factor(9) == 1.0
    z = Schedule()
    assert not z.active and FULL.active
    for t in (1, 2, 1000, 10 ** 9):
        assert z.lr_factor(t) == 1.0 and z.kl_factor(t) == 1.0
    # warm-up only / anneal only leave the other factor at exactly 1
    assert Schedule(lr_warmup_steps=3).kl_factor(1) == 1.0 and Schedule(kl_anneal_steps=3).lr_factor(1) == 1.0
    assert Schedule(lr_warmup_steps=3).lr_factor(4) == 1.0


@pytest.mark.parametrize("kw", [
    dict(lr_decay="cosine", lr_warmup_steps=4, lr_decay_steps=4),   # T <= W
    dict(lr_decay="cosine"),                                        # T = 0
    dict(lr_min_ratio=-0.1), dict(lr_min_ratio=1.5), dict(lr_min_ratio=float("nan")),
    dict(lr_warmup_steps=-1), dict(kl_anneal_steps=-2), dict(lr_decay_steps=-1),
    dict(lr_decay="linear"), dict(lr_warmup_steps=1.5),
])
def test_validation(kw):
    with pytest.raises(ValueError):
        Schedule(**kw)


def _mlp(schedule="absent", seed=0):
    kw = {} if schedule == "absent" else dict(schedule=schedule)
    tr = MlpVaeTrainer(batch_size=32, D=64, H=32, Z=4, backend="torch", seed=seed, lr=LR, kl_beta=BETA, **kw)
    X = torch.rand(320, 64, generator=torch.Generator().manual_seed(4))
    tr.bind_train_data(X, torch.arange(320, dtype=torch.int32))
    tr.set_cursor(0, 10)
    return tr


def _conv(schedule="absent", seed=0):
    kw = {} if schedule == "absent" else dict(schedule=schedule)
    tr = ConvVaeTrainer(batch_size=8, image=28, z=32, backend="torch", seed=seed, lr=LR, kl_beta=BETA, **kw)
    X = torch.rand(80, 784, generator=torch.Generator().manual_seed(5))
    tr.bind_train_data(X, torch.arange(80, dtype=torch.int32))
    tr.set_cursor(0, 10)
    return tr


def _same(a, b, steps):
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.loss_history()[:steps], b.loss_history()[:steps])
    assert a.read_state() == b.read_state() and a.read_state()["step"] == steps


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv28"])
def test_torch_backend_matches_host_driven_oracle(make):
    a, o = make(FULL), make()
    for t in range(1, 11):
        o.set_hparams(lr=LR * FULL.lr_factor(t), kl_beta=BETA * FULL.kl_factor(t))
        a.train_steps(1)
        o.train_steps(1)
        st = a.read_state()
        assert st["lr"] == LR * FULL.lr_factor(t)
        assert st["kl_beta"] == float(np.float32(BETA * FULL.kl_factor(t)))
    _same(a, o, 10)
    # evaluate() keeps the full beta: a trainer whose annealing has barely begun agrees bitwise
    Xe = torch.rand(20, a.D, generator=torch.Generator().manual_seed(6))
    b = make(Schedule(kl_anneal_steps=1000))
    b.load_state_dict(a.state_dict())
    la, _ = a.evaluate(Xe, torch.arange(20, dtype=torch.int32))
    lb, _ = b.evaluate(Xe, torch.arange(20, dtype=torch.int32))
    assert la == lb and b.read_state(eval=True)["kl_beta"] == BETA


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv28"])
def test_no_schedule_is_bitwise_the_default(make):
    a, b, z = make(None), make(), make(Schedule())
    for tr in (a, b, z):
        tr.train_steps(5)
    _same(a, b, 5)
    _same(z, b, 5)
    assert a.read_state()["lr"] == LR and a.read_state()["kl_beta"] == BETA


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv28"])
def test_resume_continues_the_schedule(make, tmp_path):
    whole, first = make(FULL, seed=1), make(FULL, seed=1)
    whole.train_steps(10)
    first.train_steps(4)
    spec = TrialSpec(group_id=0, epochs=1, lr=LR, beta=BETA, seed=1, lr_warmup_steps=4, lr_decay="cosine",
                     lr_decay_steps=12, lr_min_ratio=0.1, kl_anneal_steps=5)
    path = ckpt.save_trial(str(tmp_path), first, spec, epoch=1)
    raw = torch.load(path, weights_only=True)  # the string field survives the safe loader
    assert raw["trial"]["lr_decay"] == "cosine" and raw["trial"]["lr_decay_steps"] == 12
    assert raw["schedule"] == FULL.to_dict()
    fresh = make(seed=1)  # no schedule of its own: the checkpoint carries it
    prog = ckpt.load_latest(str(tmp_path), 0, fresh)
    assert prog["step"] == 4 and fresh.schedule == FULL
    assert fresh.read_state()["lr"] == LR * FULL.lr_factor(4)
    fresh.set_cursor(4, 10)
    fresh.train_steps(6)
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(fresh, name), getattr(whole, name)), name
    assert np.array_equal(fresh.loss_history()[4:10], whole.loss_history()[4:10])
    assert fresh.read_state()["lr"] == whole.read_state()["lr"] == LR * FULL.lr_factor(10)


def test_build_specs_cycles_lists():
    specs = build_specs(4, 2, lrs=[1e-3, 2e-3], betas=[1.0], epoch_offset=False, lr_warmups=[0, 10],
                        lr_decays=["none", "cosine", "cosine"], lr_decay_steps=[0, 100], lr_min_ratios=[0.1],
                        kl_anneals=[5, 0, 7])
    assert [s.lr_warmup_steps for s in specs] == [0, 10, 0, 10]
    assert [s.lr_decay for s in specs] == ["none", "cosine", "cosine", "none"]
    assert [s.lr_decay_steps for s in specs] == [0, 100, 0, 100]
    assert [s.lr_min_ratio for s in specs] == [0.1] * 4
    assert [s.kl_anneal_steps for s in specs] == [5, 0, 7, 5]
    assert build_specs(2, 1) == [TrialSpec(0, 1, 1e-3, 1.0, 0), TrialSpec(1, 2, 1e-3, 1.0, 1)]  # defaults unchanged
    assert specs[0].schedule().active and not build_specs(1, 1)[0].schedule().active
    # cosine without explicit steps: the runner's total step count stands in
    assert specs[2].schedule(total_steps=40) == Schedule(0, "cosine", 40, 0.1, 7)
    assert specs[1].schedule(total_steps=40).lr_decay_steps == 100
    with pytest.raises(ValueError):
        specs[2].schedule()
    with pytest.raises(ValueError):
        build_specs(1, 1, lr_min_ratios=[2.0])
    with pytest.raises(ValueError):
        build_specs(1, 1, lr_decays=["cosine"], lr_warmups=[50], lr_decay_steps=[20])


def _vae_hpo():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parse_args_schedule_flags():
    from multidisttorch_amd.hpo.trial import parse_list

    cli = _vae_hpo()
    a = cli.parse_args([])
    assert (a.lr_warmup, a.lr_decay, a.lr_decay_steps, a.lr_min_ratio, a.kl_anneal) == (None,) * 5
    a = cli.parse_args(["--lr-warmup", "100,0", "--lr-decay", "cosine,none", "--lr-decay-steps", "2000",
                        "--lr-min-ratio", "0.1", "--kl-anneal", "500"])
    assert parse_list(a.lr_warmup, int) == [100, 0] and parse_list(a.lr_decay, str) == ["cosine", "none"]
    assert parse_list(a.lr_decay_steps, int) == [2000] and parse_list(a.lr_min_ratio) == [0.1]
    assert parse_list(a.kl_anneal, int) == [500]


def test_end_to_end_cpu_runner(tmp_path):
    """One group of two replicas through the HPO runner on the CPU backend."""
    cmd = [sys.executable, "-m", "multidisttorch_amd.launch", "-n", "2", "vae-hpo.py", "--ngroups", "1", "--backend",
           "torch", "--epochs", "1", "--no-epoch-offset", "--train-samples", "256", "--test-samples", "64",
           "--no-results", "--lr-warmup", "3", "--kl-anneal", "5", "--metrics-dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    agg = json.loads(re.search(r"MDT_AGGREGATE (.*)", r.stdout).group(1))
    assert agg["failed_trials"] == []
    with open(os.path.join(str(tmp_path), "trial-0.jsonl")) as f:
        recs = [json.loads(l) for l in f if l.strip()]
    rec = [x for x in recs if x.get("epoch") == 1][-1]
    # the group's shard is the 256 rows (one sampler replica): two 128-row steps, so the
    # record carries the effective values of t = 2 beside the base ones
    s = Schedule(lr_warmup_steps=3, kl_anneal_steps=5)
    assert rec["lr_base"] == 1e-3 and rec["beta"] == 1.0
    assert rec["lr"] == 1e-3 * s.lr_factor(2) and rec["kl_beta"] == float(np.float32(s.kl_factor(2)))
