"""The table of sample scores (hpo/sample_scores.py) against literals from before the table existed: the
flags and their defaults, the refusal without ``--sample-report``, the stdout lines (plain and under the
mixture's prefix), the summary entries with their rounding and best-trial keys, and the all-off defaults."""
import contextlib
import importlib.util
import os

import pytest
import torch

from multidisttorch_amd.hpo import runner, sample_scores
from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.trial import build_specs

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _cli():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_scores", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rows_and_their_order():
    assert [s.key for s in sample_scores.SCORES] == ["prdc", "swd", "sinkhorn", "ndb"]
    assert [s.key for s in sample_scores.REPORTS] == ["sample_report", "prdc", "recon_report", "swd", "gmm", "sinkhorn", "ndb"]
    assert sample_scores.FIELDS == ("prdc_k", "swd_dirs", "sinkhorn_blur", "sinkhorn_iters", "ndb_k", "ndb_iters")


def test_flags_parse_to_the_defaults():
    a = _cli().parse_args([])
    got = {k: getattr(a, k) for k in ("prdc", "swd", "sinkhorn", "sinkhorn_iters", "ndb", "ndb_iters")}
    assert got == dict(prdc=0, swd=0, sinkhorn=0.0, sinkhorn_iters=100, ndb=0, ndb_iters=20)
    assert type(a.sinkhorn) is float and type(a.prdc) is int
    a = _cli().parse_args("--sample-report 64 --prdc 3 --swd 8 --sinkhorn 0.05 --sinkhorn-iters 20 --ndb 4 --ndb-iters 5".split())
    got = {k: getattr(a, k) for k in ("prdc", "swd", "sinkhorn", "sinkhorn_iters", "ndb", "ndb_iters")}
    assert got == dict(prdc=3, swd=8, sinkhorn=0.05, sinkhorn_iters=20, ndb=4, ndb_iters=5)
    o = runner.RunOptions()
    assert (o.prdc_k, o.swd_dirs, o.sinkhorn_blur, o.sinkhorn_iters, o.ndb_k, o.ndb_iters) == (0, 0, 0.0, 100, 0, 20)


@pytest.mark.parametrize("argv, message", [
    ("--prdc 3", "--prdc K scores the rows of the sample pass: it needs --sample-report N"),
    ("--swd 8", "--swd P scores the rows of the sample pass: it needs --sample-report N"),
    ("--sinkhorn 0.05", "--sinkhorn E scores the rows of the sample pass: it needs --sample-report N"),
    ("--ndb 4", "--ndb K bins the rows of the sample pass: it needs --sample-report N"),
])
def test_refusal_without_the_sample_pass(argv, message):
    with pytest.raises(ValueError) as e:
        _cli().parse_args(argv.split())
    assert str(e.value) == message


@pytest.mark.parametrize("argv", ["--prdc 9", "--swd 4097", "--sinkhorn 5", "--sinkhorn 0.05 --sinkhorn-iters 0", "--ndb 1",
                                  "--ndb 4 --ndb-iters 1001"])
def test_domain_checks_run_at_parse_time(argv):
    with pytest.raises(ValueError):
        _cli().parse_args(["--sample-report", "64"] + argv.split())


RESULTS = dict(
    prdc=dict(k=3, precision=0.123456789, recall=0.5, density=1.0000004, coverage=0.25),
    swd=dict(dirs=8, swd1=0.123456789, swd1_se=0.0012345678, swd2=0.2, max_w1=0.3),
    sinkhorn=dict(blur=0.05, iters=20, scale=123.456789, sinkhorn=0.123456789, w2=0.35136418, ot=1.5, marg_err=1.23456789e-05),
    ndb=dict(K=4, iters=5, ndb=2, ndb_over_k=0.5, jsd=0.123456789, missing=1, inertia=12345.6789, moved=0,
             counts_real=[1, 2], counts_fake=[2, 1]),
)
LINES = dict(
    prdc="PRDC-3: precision 0.1235 recall 0.5000 density 1.0000 coverage 0.2500",
    swd="SWD-8: W1 0.123457 +- 0.001235 W2 0.200000 max 0.300000",
    sinkhorn="Sinkhorn-0.05: S 0.123457 W2 0.351364 OT 1.500000 marg err 1.235e-05 (20 iters)",
    ndb="NDB-4: ndb 2 (0.500) JSD 0.1235 missing 1 inertia 12345.7 moved 0 (5 iters)",
)
SUMMARY = dict(
    prdc={"prdc": {"0": dict(k=3, precision=0.123457, recall=0.5, density=1.0, coverage=0.25),
                   "1": dict(k=3, precision=0.123457, recall=0.5, density=1.0, coverage=0.25)}},
    swd={"swd": {"0": dict(dirs=8, swd1=0.123457, swd1_se=0.001235, swd2=0.2, max_w1=0.3),
                 "1": dict(dirs=8, swd1=0.123457, swd1_se=0.001235, swd2=0.2, max_w1=0.3)}, "best_trial_by_swd": 0},
    sinkhorn={"sinkhorn": {"0": dict(blur=0.05, iters=20, scale=123.457, sinkhorn=0.123457, w2=0.351364, ot=1.5, marg_err=1.23457e-05),
                           "1": dict(blur=0.05, iters=20, scale=123.457, sinkhorn=0.123457, w2=0.351364, ot=1.5,
                                     marg_err=1.23457e-05)}, "best_trial_by_sinkhorn": 0},
    ndb={"ndb": {"0": dict(K=4, iters=5, ndb=2, ndb_over_k=0.5, jsd=0.123457, missing=1, inertia=12345.7, moved=0),
                 "1": dict(K=4, iters=5, ndb=2, ndb_over_k=0.5, jsd=0.123457, missing=1, inertia=12345.7, moved=0)},
         "best_trial_by_ndb_jsd": 0},
)
ON = dict(prdc=dict(prdc_k=3), swd=dict(swd_dirs=8), sinkhorn=dict(sinkhorn_blur=0.05, sinkhorn_iters=20),
          ndb=dict(ndb_k=4, ndb_iters=5))
KWARGS = dict(prdc=dict(prdc_k=3), swd=dict(swd_dirs=8), sinkhorn=dict(sinkhorn_blur=0.05, sinkhorn_iters=20),
              ndb=dict(ndb=4, ndb_iters=5, ndb_group=7))
SAMPLE = dict(mmd2=0.5, nn_acc=0.75, nn_acc_real=0.5, nn_acc_fake=1.0)


class _Trainer:
    """``evaluate_samples`` records its keywords and returns the fixed results of the scores they ask for."""

    def __init__(self):
        self._data = (torch.zeros(4, 4), torch.arange(4))

    @contextlib.contextmanager
    def averaged_weights(self):
        yield

    def evaluate_samples(self, X, idx, n, **kw):
        self.kw = kw
        on = [k for k in RESULTS if set(KWARGS[k]) & set(kw)]
        r = dict(SAMPLE, **{k: dict(RESULTS[k]) for k in on})
        if "gmm_k" in kw:
            r["gmm"] = dict(k=kw["gmm_k"], iters=kw["gmm_iters"], rows_fit=4, ll_fit=-1.0, ll_history=[-1.0], ll_test=-2.0,
                            lp_test=-3.0, gap=1.0, min_weight=0.25, sample_report=dict(SAMPLE),
                            **{k: dict(RESULTS[k]) for k in on})
        return r


class _Test:
    data = torch.zeros(8, 4)

    def __len__(self):
        return 8


class _Metrics:
    group_id = 7

    def log(self, **row):
        self.row = row


def _run(capsys, **opts):
    tr, m = _Trainer(), _Metrics()
    out = runner._sample_eval(tr, _Test(), runner.RunOptions(sample_report=8, **opts), None, m, torch.device("cpu"))
    lines = [l.split("====> Test set ", 1)[1] for l in capsys.readouterr().out.splitlines()]
    return tr, out, lines


@pytest.mark.parametrize("key", list(RESULTS))
def test_line_and_keywords_of_one_score(key, capsys):
    tr, out, lines = _run(capsys, **ON[key])
    assert tr.kw == KWARGS[key]
    assert lines == ["samples: MMD2 0.500000 1-NN acc 0.7500 (real 0.5000 gen 1.0000)", LINES[key]]
    assert list(out) == ["sample_report", key] and out[key] == RESULTS[key]


def test_every_score_and_the_mixture_prefix(capsys):
    every = {k: v for on in ON.values() for k, v in on.items()}
    tr, out, lines = _run(capsys, gmm_k=3, gmm_iters=5, **every)
    assert {k: v for k, v in tr.kw.items() if k != "fit_rows"} == dict(
        gmm_k=3, gmm_iters=5, **{k: v for kw in KWARGS.values() for k, v in kw.items()})
    assert lines == (["samples: MMD2 0.500000 1-NN acc 0.7500 (real 0.5000 gen 1.0000)"] + [LINES[k] for k in RESULTS]
                     + ["GMM-3: ll -2.0000 prior -3.0000 gap 1.0000 MMD2 0.500000 1-NN acc 0.7500"]
                     + ["GMM-3 " + LINES[k] for k in RESULTS])
    assert list(out) == ["sample_report", "prdc", "swd", "sinkhorn", "ndb", "gmm"]


def test_all_off_is_the_default_call_and_record(capsys):
    tr, out, lines = _run(capsys)
    assert tr.kw == {} and list(out) == ["sample_report"] and len(lines) == 1
    res = runner.TrialResult(group_id=0, epochs=1, shard=1, samples=8, wall_s=1.0)
    assert list(trial_record(res, runner.RunOptions())) == ["group_id", "samples", "wall_s", "failed", "iw_nll", "latent",
                                                             "test_loss_raw"]
    assert list(summarize([[trial_record(res, runner.RunOptions())]], build_specs(1, 1), runner.RunOptions())) == [
        "metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials"]


@pytest.mark.parametrize("key", list(RESULTS))
def test_summary_entry_of_one_score(key):
    opts = runner.RunOptions(sample_report=8, **ON[key])
    # two trials with equal scores, the higher group id first: the tie goes to the lower id
    recs = []
    for gid in (1, 0):
        res = runner.TrialResult(group_id=gid, epochs=1, shard=1, samples=8, wall_s=1.0)
        res.extra = {"sample_report": dict(SAMPLE), key: dict(RESULTS[key])}
        recs.append(trial_record(res, opts))
        assert list(recs[-1])[-2:] == ["sample_report", key]
    s = summarize([recs], build_specs(2, 1), opts)
    base = ["metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials", "sample_rows", "sample_report",
            "best_trial_by_mmd2"]
    assert list(s) == base + list(SUMMARY[key])
    assert {k: s[k] for k in SUMMARY[key]} == SUMMARY[key]
    assert s["sample_rows"] == 8 and s["sample_report"]["1"] == SAMPLE and s["best_trial_by_mmd2"] == 0


def test_summary_order_with_every_report_on():
    opts = runner.RunOptions(sample_report=8, recon_report=True, gmm_k=3, **{k: v for on in ON.values() for k, v in on.items()})
    res = runner.TrialResult(group_id=0, epochs=1, shard=1, samples=8, wall_s=1.0)
    gmm = dict(k=3, iters=5, rows_fit=4, ll_fit=-1.0, ll_history=[-1.0], ll_test=-2.0, lp_test=-3.0, gap=1.123456789,
               min_weight=0.25, sample_report=dict(SAMPLE, mmd2=0.123456789))
    recon = dict(mse=0.1, psnr=10.0, ssim=0.123456789, ssim_l=0.5, ssim_cs=0.25, ssim_min=0.0)
    res.extra = dict(sample_report=dict(SAMPLE), recon_report=recon, gmm=gmm, **{k: dict(v) for k, v in RESULTS.items()})
    rec = trial_record(res, opts)
    assert list(rec)[7:] == ["sample_report", "prdc", "recon_report", "swd", "gmm", "sinkhorn", "ndb"]
    s = summarize([[rec]], build_specs(1, 1), opts)
    assert list(s)[7:] == ["sample_rows", "sample_report", "best_trial_by_mmd2", "prdc", "recon_report", "best_trial_by_ssim",
                           "swd", "best_trial_by_swd", "gmm", "best_trial_by_gmm_mmd2", "sinkhorn", "best_trial_by_sinkhorn",
                           "ndb", "best_trial_by_ndb_jsd"]
    assert s["gmm"]["0"] == dict(k=3, iters=5, rows_fit=4, ll_fit=-1.0, ll_test=-2.0, lp_test=-3.0, gap=1.123457,
                                 min_weight=0.25, mmd2=0.123457, nn_acc=0.75, nn_acc_real=0.5, nn_acc_fake=1.0)
    assert s["recon_report"]["0"] == dict(mse=0.1, psnr=10.0, ssim=0.123457, ssim_l=0.5, ssim_cs=0.25, ssim_min=0.0)
