"""The Sinkhorn divergence (models/sinkhorn.py) on the CPU: the oracle's closed properties and its convergence
to exact transport, the domain, the torch backend of a trainer, the flags and the aggregate."""
import importlib.util
import itertools
import os

import pytest
import torch

from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, TrialResult
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models import sinkhorn as sk
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from tests import sinkhorn_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(real, fake, E, T):
    return sk.sinkhorn_stats(*(lambda pot, m, e: (pot, real.shape[0], m, e))(*sk.sinkhorn_rows(real, fake, E, T)), E, T)


def test_identical_sets_give_zero_and_the_divergence_is_not_negative():
    real, fake = (t.double() for t in kc.rows("uniform", (37, 29, 20)))
    same = _stats(real, real.clone(), 0.05, 40)
    assert abs(same["sinkhorn"]) <= 1e-12 * same["scale"] and same["w2"] <= 1e-6 * same["scale"] ** 0.5
    for E, T in ((0.5, 1), (0.05, 12), (0.002, 40)):
        s = _stats(real, fake, E, T)
        assert list(s) == ["blur", "iters", "scale", "sinkhorn", "w2", "ot", "marg_err"] and s["sinkhorn"] >= -1e-9
        assert s["scale"] == float(sk.sinkhorn_costs(real, fake)[3]) and (s["blur"], s["iters"]) == (E, T)


def test_marginal_error_falls_with_the_iterations():
    real, fake = (t.double() for t in kc.rows("uniform", (37, 29, 20)))
    errs = [_stats(real, fake, 0.05, T)["marg_err"] for T in (8, 16, 32, 64)]
    assert all(a > b for a, b in zip(errs, errs[1:])) and errs[-1] < 1e-3 < errs[0]


def test_small_blur_converges_to_the_optimal_assignment():
    real, fake = (t.double() for t in kc.rows("uniform", (6, 6, 3)))
    Cxy = sk.sinkhorn_costs(real, fake)[0]
    best = min(float(Cxy[torch.arange(6), torch.tensor(p)].mean()) for p in itertools.permutations(range(6)))
    s = _stats(real, fake, 0.001, 2000)
    # measured from the oracle in float64: |sinkhorn - best| = 2.563e-6 scale (E = 0.001, T = 2000; the marginals are
    # then violated by 1.3e-3); asserted with a 2x margin
    print(f"optimal assignment {best:.9f} sinkhorn {s['sinkhorn']:.9f} ot {s['ot']:.9f} gap/scale "
          f"{abs(s['sinkhorn'] - best) / s['scale']:.3e} marg_err {s['marg_err']:.3e}")
    assert abs(s["sinkhorn"] - best) <= 2 * 2.563e-6 * s["scale"]


@pytest.mark.parametrize("args,text", [((1, 9, 5, 0.05, 10), "got 1 real rows"), ((9, 16385, 5, 0.05, 10), "got 16385 generated rows"),
                                       ((9, 9, 0, 0.05, 10), "got D = 0"), ((9, 9, 65537, 0.05, 10), "got D = 65537"),
                                       ((9, 9, 5, 0.0, 10), "got 0.0"), ((9, 9, 5, 4.5, 10), "got 4.5"),
                                       ((9, 9, 5, float("nan"), 10), "got nan"), ((9, 9, 5, float("inf"), 10), "got inf"),
                                       ((9, 9, 5, 0.05, 0), "got 0"), ((9, 9, 5, 0.05, 10001), "got 10001")])
def test_domain(args, text):
    with pytest.raises(ValueError, match=text):
        sk.check_sinkhorn_args(*args)
    sk.check_sinkhorn_args(2, 16384, 1, 4.0, 1)
    sk.check_sinkhorn_args(16384, 2, 65536, 1e-6, 10000)


def test_equal_real_rows_have_no_scale():
    x = torch.ones(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="all real rows are equal"):
        _stats(x, x + 1, 0.05, 2)


def test_torch_backend_trainer_gives_the_oracle_on_its_rows():
    tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", lr=3e-3, seed=3)
    X, idx = torch.rand(64, 20, generator=torch.Generator().manual_seed(7)), torch.arange(24)
    base = tr.evaluate_samples(X, idx, 19, return_rows=True)
    r = tr.evaluate_samples(X, idx, 19, return_rows=True, sinkhorn_blur=0.05, sinkhorn_iters=12)
    assert set(r) == set(base) | {"sinkhorn", "sinkhorn_pot"} and torch.equal(r["table"], base["table"])
    assert set(tr.evaluate_samples(X, idx, 19, return_rows=True, sinkhorn_blur=0.0)) == set(base)
    case = kc.reference(r["real"], r["fake"], 0.05, 12, exact_costs=False)
    s = r["sinkhorn"]
    assert r["sinkhorn_pot"].dtype == torch.float32 and kc.check(r["sinkhorn_pot"], s["scale"], s["marg_err"], case, 0.05, 12, "torch") == s
    with pytest.raises(ValueError, match="blur"):
        tr.evaluate_samples(X, idx, 19, sinkhorn_blur=5.0)


def test_flags_need_the_sample_pass_and_their_domain():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_sinkhorn", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match="needs --sample-report"):
        mod.parse_args(["--sinkhorn", "0.05"])
    for bad in (["--sinkhorn", "5", "--sample-report", "32"], ["--sinkhorn", "0.05", "--sample-report", "16385"],
                ["--sinkhorn", "0.05", "--sinkhorn-iters", "0", "--sample-report", "32"]):
        with pytest.raises(ValueError, match="Sinkhorn"):
            mod.parse_args(bad)
    a = mod.parse_args(["--sinkhorn", "0.05", "--sinkhorn-iters", "30", "--sample-report", "32"])
    assert (a.sinkhorn, a.sinkhorn_iters) == (0.05, 30) and (mod.parse_args([]).sinkhorn, mod.parse_args([]).sinkhorn_iters) == (0.0, 100)


def test_aggregate_carries_sinkhorn_and_the_best_trial_only_under_the_option():
    w = dict(blur=0.05, iters=100, scale=52.5, sinkhorn=1.23456789, w2=1.1111, ot=9.0, marg_err=1.2345678e-5)
    on = RunOptions(sample_report=32, sinkhorn_blur=0.05)
    recs = [[dict(trial_record(TrialResult(g, 2, 128, 256, 1.5, 0.1, 0.2, failed=False,
                                           extra=dict(sample_report=dict(mmd2=0.5, nn_acc=0.5, nn_acc_real=0.5, nn_acc_fake=0.5),
                                                      sinkhorn=dict(w, ot=9.0 + g))), o)) for g in (1, 0)]
            for o in (RunOptions(sample_report=32), on)]
    assert "sinkhorn" not in recs[0][0] and list(recs[1][0])[-1] == "sinkhorn"
    s_off = summarize([recs[0]], build_specs(2, 1), RunOptions(sample_report=32))
    s_on = summarize([recs[1]], build_specs(2, 1), on)
    assert list(s_on) == list(s_off) + ["sinkhorn", "best_trial_by_sinkhorn"] and s_on["best_trial_by_sinkhorn"] == 0  # a tie: the lower id
    assert s_on["sinkhorn"]["1"] == dict(blur=0.05, iters=100, scale=52.5, sinkhorn=1.23457, w2=1.1111, ot=10.0, marg_err=1.23457e-05)
