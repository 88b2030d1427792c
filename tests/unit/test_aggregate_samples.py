"""``--sample-report`` in the run summary (hpo/aggregate.py) on hand-written
per-rank records, and one run of vae-hpo.py through the local launcher with and
without the flag. Without it every record and summary is what it was."""
import json
import os
import re
import sys

import pytest

from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, TrialResult
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.launch import launch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
METRIC = "aggregate VAE samples/sec across K concurrent HPO trials"
BASE_KEYS = ["metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials"]
SAMPLE_KEYS = ["sample_rows", "sample_report", "best_trial_by_mmd2"]


def _rep(mmd2, acc, real, fake):
    return dict(rows_real=32, rows_fake=32, mean_pair_d2=100.0, bandwidths=[25.0, 100.0, 400.0], mmd2=mmd2,
                mmd2_per_bandwidth=[mmd2, mmd2, mmd2], nn_acc=acc, nn_acc_real=real, nn_acc_fake=fake,
                nn_dist_real_to_fake=7.5, nn_dist_fake_to_real=6.25, rf_asym=0.0, sample_s=0.125)


def _rec(gid, samples, wall, failed=False, sample_report="absent", latent=None):
    r = dict(group_id=gid, samples=samples, wall_s=wall, failed=failed, iw_nll=None, latent=latent,
             test_loss_raw=None)
    if sample_report != "absent":
        r["sample_report"] = sample_report
    return r


def test_trial_record_carries_the_report_only_under_the_option():
    rep = _rep(0.0123456789, 0.75, 0.5, 1.0)
    r = TrialResult(3, 2, 128, 256, 1.5, 0.1, 0.2, failed=False, extra=dict(sample_report=rep))
    base = dict(group_id=3, samples=256, wall_s=1.5, failed=False, iw_nll=None, latent=None, test_loss_raw=None)
    assert trial_record(r, RunOptions()) == base and list(trial_record(r, RunOptions())) == list(base)
    on = trial_record(r, RunOptions(sample_report=32))
    assert on == dict(base, sample_report=rep) and list(on) == list(base) + ["sample_report"]
    bad = TrialResult(1, 0, 128, 0, 0.5, failed=True, error="boom")
    assert trial_record(bad, RunOptions(sample_report=32)) == dict(
        group_id=1, samples=0, wall_s=0.5, failed=True, iw_nll=None, latent=None, test_loss_raw=None,
        sample_report=None)
    json.dumps(on)


def test_summary_without_the_option_ignores_the_records_key():
    specs = build_specs(2, 1)
    s = summarize([[_rec(0, 256, 1.25, sample_report=_rep(0.5, 0.9, 0.8, 1.0))], [_rec(1, 512, 2.0)]], specs,
                  RunOptions())
    assert s == {"metric": METRIC, "trials": 2, "samples": 768, "wall_s": 2.0, "value": 384.0, "unit": "samples/s",
                 "failed_trials": []}
    assert list(s) == BASE_KEYS


def test_summary_with_the_option_two_ranks_of_one_trial_and_an_idle_rank():
    specs = build_specs(2, 1)
    a, b = _rep(0.0123456789, 0.7512345678, 0.5, 1.0), _rep(0.0023456712, 0.5, 0.40625, 0.59375)
    lat = dict(kl=3.0, active_units=2, mi=1.0, tc=0.5, dwkl=1.5)
    gathered = [[_rec(0, 256, 1.5, sample_report=a, latent=lat)], [_rec(0, 250, 2.25, sample_report=a, latent=lat)],
                None, [_rec(1, 128, 1.0, sample_report=b, latent=lat)], []]
    s = summarize(gathered, specs, RunOptions(sample_report=32, latent_report=True))
    assert s["sample_rows"] == 32 and s["best_trial_by_mmd2"] == 1
    assert s["sample_report"] == {"0": {"mmd2": 0.012346, "nn_acc": 0.751235, "nn_acc_real": 0.5, "nn_acc_fake": 1.0},
                                  "1": {"mmd2": 0.002346, "nn_acc": 0.5, "nn_acc_real": 0.40625,
                                        "nn_acc_fake": 0.59375}}
    assert list(s) == BASE_KEYS + ["latent"] + SAMPLE_KEYS            # after the latent block
    assert list(s["sample_report"]["0"]) == ["mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake"]
    assert s["trials"] == 2 and s["samples"] == 378
    assert list(summarize(gathered, specs, RunOptions(sample_report=32))) == BASE_KEYS + SAMPLE_KEYS


def test_a_tie_goes_to_the_lower_trial_and_a_failed_trial_is_absent():
    specs = build_specs(3, 1)
    rep = _rep(0.25, 0.5, 0.5, 0.5)
    gathered = [[_rec(0, 0, 0.5, failed=True, sample_report=None)], [_rec(2, 64, 0.75, sample_report=rep)],
                [_rec(1, 64, 1.0, sample_report=rep)]]
    s = summarize(gathered, specs, RunOptions(sample_report=16))
    assert s["best_trial_by_mmd2"] == 1 and list(s["sample_report"]) == ["1", "2"] and s["failed_trials"] == [0]
    neg = summarize([[_rec(0, 64, 1.0, sample_report=_rep(-0.001, 0.5, 0.5, 0.5))],
                     [_rec(1, 64, 1.0, sample_report=rep)]], build_specs(2, 1), RunOptions(sample_report=16))
    assert neg["best_trial_by_mmd2"] == 0  # the unbiased estimate may be negative: lowest, not nearest zero


def test_no_trial_with_a_report():
    s = summarize([[_rec(0, 0, 0.5, failed=True, sample_report=None)], [_rec(1, 32, 0.25, failed=True)]],
                  build_specs(2, 1), RunOptions(sample_report=8))
    assert s == {"metric": METRIC, "trials": 2, "samples": 32, "wall_s": 0.5, "value": 64.0, "unit": "samples/s",
                 "failed_trials": [0, 1], "sample_rows": 8, "sample_report": {}, "best_trial_by_mmd2": None}


def _cli(tmp_path, name, *extra):
    mdir = os.path.join(str(tmp_path), name)
    cmd = [sys.executable, os.path.join(ROOT, "vae-hpo.py"), "--backend", "torch", "--synthetic", "--train-samples",
           "256", "--test-samples", "64", "--epochs", "1", "--ngroups", "1", "--no-results", "--metrics-dir", mdir,
           *extra]
    old = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        rc, outs = launch(cmd, 1, emulate="torchrun", timeout=300, capture=True,
                          extra_env={"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    finally:
        os.chdir(old)
    out = outs[0] or ""
    return rc, out, mdir


def test_cli_reports_samples_only_when_asked(tmp_path):
    rc, out, mdir = _cli(tmp_path, "on", "--sample-report", "32")
    assert rc == 0, out[-4000:]
    m = re.search(r"====> Test set samples: MMD2 (-?[0-9.]+) 1-NN acc ([0-9.]+) \(real ([0-9.]+) gen ([0-9.]+)\)$",
                  out, re.M)
    assert m, out[-2000:]
    mmd2, acc, real, gen = (float(g) for g in m.groups())
    assert 0.0 <= acc <= 1.0 and abs(acc - (real + gen) / 2) < 1e-4 and mmd2 > -1.0
    agg = json.loads(re.search(r"MDT_AGGREGATE (.*)", out).group(1))
    assert agg["sample_rows"] == 32 and agg["best_trial_by_mmd2"] == 0 and list(agg)[-3:] == SAMPLE_KEYS
    assert set(agg["sample_report"]) == {"0"}
    assert set(agg["sample_report"]["0"]) == {"mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake"}
    assert abs(agg["sample_report"]["0"]["mmd2"] - mmd2) < 1e-6 and abs(agg["sample_report"]["0"]["nn_acc"] - acc) < 1e-4
    with open(os.path.join(mdir, "aggregate.json")) as f:
        assert json.load(f) == agg
    with open(os.path.join(mdir, "trial-0.jsonl")) as f:
        recs = [json.loads(l) for l in f]
    ev = [r for r in recs if r.get("event") == "sample_eval"]
    assert len(ev) == 1 and ev[0]["sample_s"] > 0 and ev[0]["rows_real"] == 32 and ev[0]["rows_fake"] == 32
    assert len(ev[0]["bandwidths"]) == 3 and len(ev[0]["mmd2_per_bandwidth"]) == 3 and ev[0]["rf_asym"] < 1e-4

    rc0, out0, mdir0 = _cli(tmp_path, "off")
    assert rc0 == 0, out0[-4000:]
    assert "samples:" not in out0 and "sample_report" not in out0 and "best_trial_by_mmd2" not in out0
    with open(os.path.join(mdir0, "trial-0.jsonl")) as f:
        assert not [l for l in f if "sample_eval" in l or "mmd2" in l]
    # everything but the pass's line is what the run prints without the flag
    drop = ("Done. time", "MDT_AGGREGATE", "Test set samples", "master at", "[Gloo]")  # timings, the port, the new line
    log = re.compile(r"^\[[WIE]\d{4} ")  # c10d's timestamped stderr lines: the launcher merges the streams
    strip = lambda s: [l for l in s.splitlines() if not any(d in l for d in drop) and not log.match(l)]
    assert strip(out) == strip(out0)


@pytest.mark.parametrize("n,text", [(1, "got 1 real rows"), (-3, "got -3 real rows"), (40000, "got 40000 real rows"),
                                    (65, "exceeds --test-samples 64")])
def test_cli_rejects_a_bad_count_at_parse(n, text):
    import importlib.util

    spec = importlib.util.spec_from_file_location("vae_hpo_cli_samples", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match=re.escape(text)):
        mod.parse_args(["--sample-report", str(n), "--test-samples", "64"])
    assert mod.parse_args([]).sample_report == 0 and mod.parse_args(["--sample-report", "64"]).sample_report == 64
