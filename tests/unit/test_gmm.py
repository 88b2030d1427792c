"""The mixture prior (models/gmm.py) on the CPU: the fit on a planted mixture, the stratified draw, the dead-component
rule, the pivot check, the flag, and the torch backend of both trainers."""
import importlib.util
import os

import pytest
import torch

from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, TrialResult
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models import gmm
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from tests import gmm_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_fit_reaches_the_planted_likelihood():
    z, planted = gc.planted(600, 5, 3)
    fit = gmm.gmm_fit(z.double(), 3, 50)
    h = fit["ll_history"]
    assert h.shape == (51,) and bool((h[1:] >= h[:-1] - 1e-9).all())   # EM never lowers the likelihood
    assert float(h[-1]) >= float(gmm.gmm_score(z.double(), planted).mean()) - 1e-3
    assert torch.equal(h[-1], gmm.gmm_score(z.double(), fit).mean()) and float(fit["pi"].sum()) == pytest.approx(1.0)


def test_sample_counts_follow_the_largest_remainder():
    # 10 * pi = 4.5, 2.5, 2.5, 0.5: floors 4, 2, 2, 0 and two rows left for four equal remainders, the lower k first
    assert gmm.gmm_counts([0.45, 0.25, 0.25, 0.05], 10).tolist() == [5, 3, 2, 0]
    assert gmm.gmm_counts([0.26, 0.37, 0.37], 10).tolist() == [2, 4, 4]
    p = dict(pi=torch.tensor([0.45, 0.25, 0.25, 0.05], dtype=torch.float64), mu=torch.arange(4.0)[:, None] * torch.ones(4, 2) * 100,
             cov=torch.eye(2).expand(4, 2, 2))
    s = gmm.gmm_sample(p, 10, 3)
    assert s.shape == (10, 2) and s.dtype == torch.float32 and torch.equal(s, gmm.gmm_sample(p, 10, 3))
    assert (s[:, 0] / 100).round().long().tolist() == [0] * 5 + [1] * 3 + [2] * 2   # rows ordered by component


def test_dead_component_keeps_its_mean_and_covariance():
    z = gc.planted(130, 4, 2)[0].double()
    pi, mu, cov = gmm.gmm_init(z, 3)
    mu[2] += 1e3
    r = gmm.gmm_estep(z, mu, *gmm.gmm_prepare(pi, mu, cov))[0]
    pi2, mu2, cov2 = gmm.gmm_mstep(z, r, mu, cov)
    assert float(pi2[2]) == 0.0 and torch.equal(mu2[2], mu[2]) and torch.equal(cov2[2], cov[2])
    assert not torch.equal(mu2[0], mu[0]) and float(pi2.sum()) == pytest.approx(1.0)


def test_prepare_raises_on_an_indefinite_covariance():
    pi, mu = torch.full((2,), 0.5, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    cov = torch.stack([torch.eye(3, dtype=torch.float64), torch.diag(torch.tensor([1.0, -1e-3, 1.0], dtype=torch.float64))])
    with pytest.raises(ValueError, match=r"not positive definite \(components \[1\]\)"):
        gmm.gmm_prepare(pi, mu, cov, reg=0.0)
    gmm.gmm_prepare(pi, mu, cov, reg=2e-3)


def test_flag_needs_the_sample_pass_and_its_domain():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_gmm", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match="needs --sample-report"):
        mod.parse_args(["--gmm", "3"])
    for bad in (["--gmm", "33", "--sample-report", "64"], ["--gmm", "3", "--gmm-iters", "1001", "--sample-report", "64"]):
        with pytest.raises(ValueError, match="mixture prior"):
            mod.parse_args(bad)
    a = mod.parse_args(["--gmm", "3", "--sample-report", "32"])
    assert (mod.parse_args([]).gmm, a.gmm, a.gmm_iters) == (0, 3, 50)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_torch_backend_trainers_return_the_report(kind):
    if kind == "mlp":
        tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", lr=3e-3, seed=3)
        X = torch.rand(64, 20, generator=torch.Generator().manual_seed(7))
    else:
        tr = ConvVaeTrainer(batch_size=16, image=28, z=8, backend="torch", device="cpu", seed=3)
        X = torch.rand(64, 784, generator=torch.Generator().manual_seed(7))
    idx = torch.arange(24)
    base = tr.evaluate_samples(X, idx, 19, return_rows=True, swd_dirs=4)
    r = tr.evaluate_samples(X, idx, 19, return_rows=True, swd_dirs=4, gmm_k=3, gmm_iters=5, fit_rows=(X, torch.arange(64)))
    assert set(r) == set(base) | {"gmm", "gmm_params", "gmm_fake", "gmm_fit_z", "gmm_test_z"}
    assert torch.equal(r["table"], base["table"]) and r["swd"] == base["swd"]
    g = r["gmm"]
    assert list(g) == ["k", "iters", "rows_fit", "ll_fit", "ll_history", "ll_test", "lp_test", "gap", "min_weight",
                       "sample_report", "swd"]
    fit = gmm.gmm_fit(r["gmm_fit_z"], 3, 5)
    assert g["ll_history"] == [float(v) for v in fit["ll_history"]] and g["rows_fit"] == 64
    assert g["ll_test"] == pytest.approx(float(gmm.gmm_score(r["gmm_test_z"], fit).double().mean()), abs=1e-12)
    assert g["gap"] == g["ll_test"] - g["lp_test"] and r["gmm_fake"].shape == r["fake"].shape
    with pytest.raises(ValueError, match="fit_rows"):
        tr.evaluate_samples(X, idx, 19, gmm_k=3)


def test_aggregate_carries_gmm_and_the_best_trial_only_under_the_option():
    rep = dict(mmd2=0.5, nn_acc=0.5, nn_acc_real=0.5, nn_acc_fake=0.5)
    g = dict(k=3, iters=50, rows_fit=256, ll_fit=-3.0, ll_test=-3.12345678, lp_test=-4.0, gap=0.87654322, min_weight=0.1)
    recs = [[dict(trial_record(TrialResult(t, 2, 128, 256, 1.5, 0.1, 0.2, failed=False,
                                           extra=dict(sample_report=rep, gmm=dict(g, sample_report=dict(rep, mmd2=0.3 - 0.1 * t)))), o))
             for t in (0, 1)] for o in (RunOptions(sample_report=32), RunOptions(sample_report=32, gmm_k=3))]
    assert "gmm" not in recs[0][0] and list(recs[1][0])[-1] == "gmm"
    s_off = summarize([recs[0]], build_specs(2, 1), RunOptions(sample_report=32))
    s_on = summarize([recs[1]], build_specs(2, 1), RunOptions(sample_report=32, gmm_k=3))
    assert list(s_on) == list(s_off) + ["gmm", "best_trial_by_gmm_mmd2"] and s_on["best_trial_by_gmm_mmd2"] == 1
    assert s_on["gmm"]["0"] == dict(k=3, iters=50, rows_fit=256, ll_fit=-3.0, ll_test=-3.123457, lp_test=-4.0,
                                    gap=0.876543, min_weight=0.1, **dict(rep, mmd2=0.3))
