"""The sliced Wasserstein distance (models/swd.py) on the CPU: the segment form against the na*nb-cell form,
two closed cases, the directions, the domain, the torch backend of a trainer, the flag and the aggregate."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, TrialResult
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models import swd
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from tests import swd_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize("shape", [(3, 2, 5, 3), (37, 29, 20, 5), (130, 257, 33, 33), (128, 128, 784, 32)])
def test_segments_are_the_cell_form(shape):
    (na, nb, _, _), (real, fake, dirs, proj, table) = shape, wc.case("uniform", shape)
    assert swd.swd_segments(na, nb)[2].numel() == na + nb - math.gcd(na, nb)
    pu = torch.cat([real, fake]).double() @ dirs.double().t()
    sr, sf = pu[:na].sort(0).values, pu[na:].sort(0).values
    assert torch.allclose(proj, torch.cat([sr, sf]).t(), rtol=0, atol=1e-13)
    t = torch.arange(na * nb)
    d = proj[:, :na][:, t // nb] - proj[:, na:][:, t // na]
    assert torch.allclose(table, torch.stack([d.abs().mean(1), (d * d).mean(1)], 1), rtol=1e-12, atol=0)


def test_two_closed_cases():
    real, _, dirs, _, _ = wc.case("uniform", (37, 29, 20, 5))
    real, dirs = real.double(), dirs.double()
    assert not bool(swd.swd_rows(real, real[torch.randperm(37)], dirs)[1].any())
    c = torch.linspace(-1, 1, 20, dtype=torch.float64)
    shift = dirs @ c
    table = swd.swd_rows(real, real + c, dirs)[1]
    assert torch.allclose(table, torch.stack([shift.abs(), shift ** 2], 1), rtol=1e-12, atol=1e-15)
    s = swd.swd_stats(table)
    assert list(s) == ["dirs", "swd1", "swd1_se", "swd2", "max_w1"] and s["dirs"] == 5
    assert s["swd1_se"] == pytest.approx(float(shift.abs().std()) / math.sqrt(5)) and swd.swd_stats(table[:1])["swd1_se"] == 0.0
    assert s["swd2"] == pytest.approx(math.sqrt(float((shift ** 2).mean()))) and s["max_w1"] == float(shift.abs().max())


def test_directions_are_unit_and_a_function_of_the_seed():
    d = swd.swd_directions(7, 33, 5)
    assert d.shape == (7, 33) and d.dtype == np.float32
    np.testing.assert_allclose((d.astype(np.float64) ** 2).sum(1), 1.0, rtol=0, atol=33 * 2.0 ** -24)
    assert np.array_equal(d, swd.swd_directions(7, 33, 5)) and not np.array_equal(d, swd.swd_directions(7, 33, 6))


@pytest.mark.parametrize("args,text", [((1, 9, 5, 3), "got 1 real rows"), ((9, 16385, 5, 3), "got 16385 generated rows"),
                                       ((9, 9, 0, 3), "got D = 0"), ((9, 9, 65537, 3), "got D = 65537"),
                                       ((9, 9, 5, 0), "got 0"), ((9, 9, 5, 4097), "got 4097")])
def test_domain(args, text):
    with pytest.raises(ValueError, match=text):
        swd.check_swd_args(*args)
    swd.check_swd_args(2, 16384, 1, 1)
    swd.check_swd_args(16384, 2, 65536, 4096)


def test_torch_backend_trainer_gives_the_oracle_on_its_rows():
    tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", lr=3e-3, seed=3)
    X, idx = torch.rand(64, 20, generator=torch.Generator().manual_seed(7)), torch.arange(24)
    base = tr.evaluate_samples(X, idx, 19, return_rows=True)
    r = tr.evaluate_samples(X, idx, 19, return_rows=True, swd_dirs=6)
    assert set(r) == set(base) | {"swd", "swd_table", "swd_proj"} and torch.equal(r["table"], base["table"])
    dirs = torch.from_numpy(swd.swd_directions(6, 20, 3))
    proj, table = swd.swd_rows(r["real"].double(), r["fake"].double(), dirs.double())
    pb, tb = wc.float_bounds(r["real"], r["fake"], dirs, table)
    assert r["swd_table"].dtype == torch.float32 and r["swd"] == swd.swd_stats(r["swd_table"])
    assert bool(((r["swd_proj"].double() - proj).abs() <= pb).all()) and bool(((r["swd_table"].double() - table).abs() <= tb).all())
    with pytest.raises(ValueError, match="directions"):
        tr.evaluate_samples(X, idx, 19, swd_dirs=4097)


def test_flag_needs_the_sample_pass_and_its_domain():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_swd", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match="needs --sample-report"):
        mod.parse_args(["--swd", "64"])
    for bad in (["--swd", "4097", "--sample-report", "32"], ["--swd", "64", "--sample-report", "16385"]):
        with pytest.raises(ValueError, match="sliced Wasserstein"):
            mod.parse_args(bad)
    assert mod.parse_args([]).swd == 0 and mod.parse_args(["--swd", "64", "--sample-report", "32"]).swd == 64


def test_aggregate_carries_swd_and_the_best_trial_only_under_the_option():
    w = dict(dirs=64, swd1=0.51234567, swd1_se=0.01, swd2=0.6, max_w1=0.9)
    recs = [[dict(trial_record(TrialResult(g, 2, 128, 256, 1.5, 0.1, 0.2, failed=False,
                                           extra=dict(sample_report=dict(mmd2=0.5, nn_acc=0.5, nn_acc_real=0.5, nn_acc_fake=0.5),
                                                      swd=dict(w, max_w1=0.9 + g))), o)) for g in (1, 0)]
            for o in (RunOptions(sample_report=32), RunOptions(sample_report=32, swd_dirs=64))]
    assert "swd" not in recs[0][0] and list(recs[1][0])[-1] == "swd"
    s_off = summarize([recs[0]], build_specs(2, 1), RunOptions(sample_report=32))
    s_on = summarize([recs[1]], build_specs(2, 1), RunOptions(sample_report=32, swd_dirs=64))
    assert list(s_on) == list(s_off) + ["swd", "best_trial_by_swd"] and s_on["best_trial_by_swd"] == 0   # a tie: the lower id
    assert s_on["swd"]["1"] == dict(dirs=64, swd1=0.512346, swd1_se=0.01, swd2=0.6, max_w1=1.9)
