"""PRDC on k-NN radii (models/prdc.py) on the CPU: the definition against a plain
double loop, two closed cases, chunking, the torch backends of both trainers,
the domain and the flag, and the aggregate's keys."""
import importlib.util
import os

import pytest
import torch

from multidisttorch_amd.data.datasets import synthetic_images
from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, TrialResult
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models import prdc
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from tests import sample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _loop_rows(real, fake, k):
    """The definition, row by row in Python floats."""
    d2 = lambda a, b: sum((float(x) - float(y)) ** 2 for x, y in zip(a, b))
    sets = (real.tolist(), fake.tolist())
    rad = [[sorted(d2(a, b) for j, b in enumerate(X) if j != i)[k - 1] for i, a in enumerate(X)] for X in sets]
    rows = []
    for s, X in enumerate(sets):
        Y, o = sets[1 - s], 1 - s
        for i, a in enumerate(X):
            dx = [d2(a, b) for b in Y]
            # a real row against the fake radii, a fake row against the real ones
            cnt = sum(1 for j, v in enumerate(dx) if v <= rad[o][j])
            rows.append([rad[s][i], float(cnt), min(dx)])
    return torch.tensor(rows, dtype=torch.float64)


@pytest.mark.parametrize("shape,k", [((7, 5, 3), 2), ((12, 9, 1), 3), ((4, 6, 2), 3)], ids=["7x5x3", "ties-D1", "4x6x2"])
def test_rows_are_the_definition(shape, k):
    real, fake = sc.lattice(*shape)  # exact in float64 either way: the comparison is bitwise
    real, fake = real.double(), fake.double()
    assert torch.equal(prdc.prdc_rows(real, fake, k), _loop_rows(real, fake, k))


def test_two_closed_cases():
    real, _ = sc.uniform(40, 40, 6)
    same = prdc.prdc_stats(prdc.prdc_rows(real.double(), real[torch.randperm(40)].double(), 3), 40, 40, 3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] > 0 and same["k"] == 3
    far = prdc.prdc_stats(prdc.prdc_rows(real.double(), real.double() + 100.0, 3), 40, 40, 3)
    assert far == dict(k=3, precision=0.0, recall=0.0, density=0.0, coverage=0.0)


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunked_equals_unchunked(chunk):
    real, fake = sc.lattice(37, 29, 20)
    assert torch.equal(prdc.prdc_rows(real, fake, 3, chunk=chunk), prdc.prdc_rows(real, fake, 3))


def _mlp():
    tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", lr=3e-3, seed=3)
    return tr, torch.rand(64, 20, generator=torch.Generator().manual_seed(7))


def _conv():
    return ConvVaeTrainer(batch_size=8, image=28, z=32, device="cpu", backend="torch", seed=3), synthetic_images(32, seed=3)


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_torch_backend_trainers_give_the_oracle_on_their_rows(make):
    tr, X = make()
    idx = torch.arange(24)
    base = tr.evaluate_samples(X, idx, 19, return_rows=True)
    r = tr.evaluate_samples(X, idx, 19, return_rows=True, prdc_k=3)
    assert set(r) == set(base) | {"prdc", "prdc_table"} and torch.equal(r["table"], base["table"])
    assert set(tr.evaluate_samples(X, idx, 19, prdc_k=3)) == set(tr.evaluate_samples(X, idx, 19)) | {"prdc"}
    real, fake = r["real"].double(), r["fake"].double()
    o, t = prdc.prdc_rows(real, fake, 3), r["prdc_table"]
    assert t.shape == (43, 3) and t.dtype == torch.float32
    assert list(r["prdc"]) == ["k", "precision", "recall", "density", "coverage"] and r["prdc"] == prdc.prdc_stats(t, 24, 19, 3)
    # float32 sums of D squared float32 differences: relative error gamma_{D+2} per distance, hence per order statistic
    g = sc.gamma(real.shape[1] + 2)
    assert torch.allclose(t[:, [0, 2]].double(), o[:, [0, 2]], rtol=g, atol=0)
    # and a count inside what thresholds moved by that much both ways admit
    d2 = ((real[:, None] - fake[None]) ** 2).sum(-1)
    lo, hi = d2 * (1 + g), d2 * (1 - g)
    rr, rf = o[:24, 0], o[24:, 0]
    cnt_lo = torch.cat([(lo <= rf[None] * (1 - g)).sum(1), (lo <= rr[:, None] * (1 - g)).sum(0)])
    cnt_hi = torch.cat([(hi <= rf[None] * (1 + g)).sum(1), (hi <= rr[:, None] * (1 + g)).sum(0)])
    assert bool(((cnt_lo <= t[:, 1]) & (t[:, 1] <= cnt_hi)).all())


@pytest.mark.parametrize("args,text", [((9, 9, 5, 0), "got k = 0"), ((9, 9, 5, 9), "got k = 9"),
                                       ((3, 9, 5, 3), "got 3 real rows"), ((9, 3, 5, 3), "got 3 generated rows"),
                                       ((9, 32769, 5, 3), "got 32769 generated rows"), ((9, 9, 0, 3), "got D = 0")])
def test_domain(args, text):
    with pytest.raises(ValueError, match=text):
        prdc.check_prdc_args(*args)
    prdc.check_prdc_args(4, 4, 1, 3)


def test_flag_needs_the_sample_pass_and_its_domain():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_prdc", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match="needs --sample-report"):
        mod.parse_args(["--prdc", "5"])
    for bad in (["--prdc", "9", "--sample-report", "32"], ["--prdc", "5", "--sample-report", "5"]):
        with pytest.raises(ValueError, match="PRDC"):
            mod.parse_args(bad)
    assert mod.parse_args([]).prdc == 0 and mod.parse_args(["--prdc", "5", "--sample-report", "6"]).prdc == 5


def test_aggregate_carries_prdc_only_under_the_option():
    p = dict(k=5, precision=0.51234567, recall=0.25, density=1.23456789, coverage=0.75)
    res = TrialResult(0, 2, 128, 256, 1.5, 0.1, 0.2, failed=False, extra=dict(sample_report=dict(mmd2=0.5), prdc=p))
    off, on = RunOptions(sample_report=32), RunOptions(sample_report=32, prdc_k=5)
    assert "prdc" not in trial_record(res, off) and list(trial_record(res, on))[-1] == "prdc"
    rec = dict(trial_record(res, on), sample_report=dict(mmd2=0.5, nn_acc=0.5, nn_acc_real=0.5, nn_acc_fake=0.5))
    s_off, s_on = (summarize([[rec]], build_specs(1, 1), o) for o in (off, on))
    assert list(s_on) == list(s_off) + ["prdc"] and not any("best_trial_by_p" in k for k in s_on)
    assert s_on["prdc"] == {"0": dict(k=5, precision=0.512346, recall=0.25, density=1.234568, coverage=0.75)}
