"""The run summary (hpo/aggregate.py) on hand-written per-rank records. The
expected dicts are written out from the rules the summary has always followed:
samples once per trial (the minimum over its ranks), the maximum wall over all
ranks, values rounded to 4 places, optional keys only under their options."""
import json

from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, TrialResult
from multidisttorch_amd.hpo.trial import build_specs

METRIC = "aggregate VAE samples/sec across K concurrent HPO trials"
BASE_KEYS = ["metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials"]


def _rec(gid, samples, wall, failed=False, iw_nll=None, latent=None, test_loss_raw=None):
    return dict(group_id=gid, samples=samples, wall_s=wall, failed=failed, iw_nll=iw_nll, latent=latent,
                test_loss_raw=test_loss_raw)


def _latent(kl, au, mi, tc, dwkl, **more):
    return dict(kl=kl, active_units=au, mi=mi, tc=tc, dwkl=dwkl, kl_per_dim=[kl / 2, kl / 2], latent_s=0.125, **more)


def test_trial_record_names_its_fields():
    r = TrialResult(3, 2, 128, 256, 1.5, 0.1, 0.2, failed=False,
                    extra=dict(iw_nll=99.5, iw_neg_elbo=101.0, iw_samples=2, iw_s=0.01, latent={"kl": 1.0},
                               test_loss_raw=104.0))
    assert trial_record(r, RunOptions()) == dict(group_id=3, samples=256, wall_s=1.5, failed=False, iw_nll=99.5,
                                                 latent={"kl": 1.0}, test_loss_raw=104.0)
    bad = TrialResult(1, 0, 128, 0, 0.5, failed=True, error="boom")
    assert trial_record(bad, RunOptions(iw_samples=2, latent_report=True)) == dict(
        group_id=1, samples=0, wall_s=0.5, failed=True, iw_nll=None, latent=None, test_loss_raw=None)
    json.dumps(trial_record(r, RunOptions()))  # plain data: it crosses all_gather_object and json


def test_nothing_enabled():
    specs = build_specs(2, 1)
    s = summarize([[_rec(0, 256, 1.25)], [_rec(1, 512, 2.0)]], specs, RunOptions())
    assert s == {"metric": METRIC, "trials": 2, "samples": 768, "wall_s": 2.0, "value": 384.0, "unit": "samples/s",
                 "failed_trials": []}
    assert list(s) == BASE_KEYS


def test_everything_enabled_two_ranks_of_one_trial_and_a_single_rank_trial():
    specs = build_specs(2, 1, free_bits="0,0.05", tc_weight="0,0.5", ema_decay="0,0.99")
    opts = RunOptions(binarize="static", report_objective=("free_bits", "tc_weight", "ema_decay"), iw_samples=2,
                      latent_report=True)
    lat0 = _latent(12.345678, 7, 1.23456, 0.54321, 10.567891)
    lat1 = _latent(9.87654, 5, 2.000049, 0.25, 7.62649, free_bits=0.05, below_floor=3)
    gathered = [[_rec(0, 256, 1.5, iw_nll=101.23456, latent=lat0)],
                [_rec(0, 250, 2.25, iw_nll=101.23456, latent=lat0)],
                [_rec(1, 128, 1.0, iw_nll=99.87654, latent=lat1, test_loss_raw=105.123456)]]
    s = summarize(gathered, specs, opts)
    assert s == {
        "metric": METRIC, "trials": 2, "samples": 378, "wall_s": 2.25, "value": 168.0, "unit": "samples/s",
        "failed_trials": [], "binarize": "static",
        "free_bits": {"0": 0.0, "1": 0.05}, "tc_weight": {"0": 0.0, "1": 0.5}, "ema_decay": {"0": 0.0, "1": 0.99},
        "test_loss_raw": {"1": 105.1235},
        "iw_samples": 2, "iw_nll": {"0": 101.2346, "1": 99.8765}, "best_trial_by_iw_nll": 1,
        "latent": {"0": {"kl": 12.3457, "active_units": 7, "mi": 1.2346, "tc": 0.5432, "dwkl": 10.5679},
                   "1": {"kl": 9.8765, "active_units": 5, "mi": 2.0, "tc": 0.25, "dwkl": 7.6265, "below_floor": 3}}}
    assert list(s) == BASE_KEYS + ["binarize", "free_bits", "tc_weight", "ema_decay", "test_loss_raw", "iw_samples",
                                   "iw_nll", "best_trial_by_iw_nll", "latent"]
    assert list(s["latent"]["1"]) == ["kl", "active_units", "mi", "tc", "dwkl", "below_floor"]
    assert isinstance(s["latent"]["0"]["active_units"], int) and isinstance(s["samples"], int)
    # the order of report_objective is not the order of the keys: that is the table's
    swapped = RunOptions(binarize="static", report_objective=("ema_decay", "free_bits"), iw_samples=2)
    assert list(summarize(gathered, specs, swapped)) == BASE_KEYS + [
        "binarize", "free_bits", "ema_decay", "test_loss_raw", "iw_samples", "iw_nll", "best_trial_by_iw_nll"]


def test_a_failed_trial_is_absent_from_the_maps_and_the_best_is_chosen_among_the_rest():
    specs = build_specs(3, 1, ema_decay=0.9)
    opts = RunOptions(report_objective=("ema_decay",), iw_samples=2, latent_report=True)
    lat = _latent(3.0, 2, 1.0, 0.5, 1.5)
    gathered = [[_rec(0, 0, 0.5, failed=True)],
                [_rec(1, 64, 1.0, iw_nll=100.5, latent=lat, test_loss_raw=103.25)],
                [_rec(2, 64, 0.75, iw_nll=100.5, latent=lat, test_loss_raw=103.0)]]
    s = summarize(gathered, specs, opts)
    small = {"kl": 3.0, "active_units": 2, "mi": 1.0, "tc": 0.5, "dwkl": 1.5}
    assert s == {"metric": METRIC, "trials": 3, "samples": 128, "wall_s": 1.0, "value": 128.0, "unit": "samples/s",
                 "failed_trials": [0], "ema_decay": {"0": 0.9, "1": 0.9, "2": 0.9},
                 "test_loss_raw": {"1": 103.25, "2": 103.0}, "iw_samples": 2, "iw_nll": {"1": 100.5, "2": 100.5},
                 "best_trial_by_iw_nll": 1,  # a tie goes to the lower trial
                 "latent": {"1": small, "2": small}}
    assert list(s) == BASE_KEYS + ["ema_decay", "test_loss_raw", "iw_samples", "iw_nll", "best_trial_by_iw_nll",
                                   "latent"]


def test_no_trial_with_an_iw_value():
    s = summarize([[_rec(0, 0, 0.5, failed=True)], [_rec(1, 32, 0.25, failed=True)]], build_specs(2, 1),
                  RunOptions(iw_samples=4, latent_report=True))
    assert s == {"metric": METRIC, "trials": 2, "samples": 32, "wall_s": 0.5, "value": 64.0, "unit": "samples/s",
                 "failed_trials": [0, 1], "iw_samples": 4, "iw_nll": {}, "best_trial_by_iw_nll": None, "latent": {}}


def test_an_idle_rank_contributes_nothing():
    for idle in ([], None):
        s = summarize([[_rec(0, 100, 1.0)], idle, [_rec(1, 100, 4.0), _rec(2, 200, 4.0)]], build_specs(3, 1),
                      RunOptions())
        assert s == {"metric": METRIC, "trials": 3, "samples": 400, "wall_s": 4.0, "value": 100.0,
                     "unit": "samples/s", "failed_trials": []}
    assert summarize([[], None], build_specs(1, 1), RunOptions())["trials"] == 0
