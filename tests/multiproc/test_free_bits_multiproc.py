"""``vae-hpo.py --free-bits 0,0.05`` over two concurrent trials (gloo, torch
backend): the aggregate carries every trial's floor, the floored trial's
training loss is the clamped objective, and a run without the flag says
nothing about it and prints what ``--free-bits 0`` prints."""
import json
import os
import re
import sys

from multidisttorch_amd.launch import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLI = os.path.join(ROOT, "vae-hpo.py")
ENV = {"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "PYTHONPATH": ROOT}
COMMON = ["--ngroups", "2", "--epochs", "1", "--no-epoch-offset", "--backend", "torch", "--synthetic",
          "--train-samples", "512", "--test-samples", "256", "--batch-size", "64", "--no-results", "--metrics-dir", "m",
          "--beta", "4"]
# the aggregate keys of a run without extensions
DEFAULT_KEYS = ["metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials"]


def _launch(tmp_path, *args, rc_ok=True):
    old = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        rc, outs = launch([sys.executable, CLI] + COMMON + list(args), 2, emulate="torchrun", timeout=300,
                          extra_env=ENV, capture=True)
    finally:
        os.chdir(old)
    text = "\n".join(o or "" for o in outs)
    if not rc_ok:
        return rc, text
    assert rc == 0, text[-4000:]
    return text, json.loads(re.search(r"MDT_AGGREGATE (.*)", text).group(1))


def _stable(text):
    """stdout without what differs from run to run: the wall-clock figures (the
    Done lines, the aggregate's rates) and the rendezvous port."""
    keep = [l for l in text.splitlines() if "Done. time" not in l and "MDT_AGGREGATE" not in l and "[mdt]" not in l
            and "master at" not in l and not re.match(r"\[[WEI]\d{4} ", l)]  # (and c10d's timestamped log lines)
    return sorted(keep)


def _epochs(tmp_path, g):
    with open(tmp_path / "m" / f"trial-{g}.jsonl") as f:
        return [r for r in map(json.loads, f) if "epoch" in r]


def test_two_trials_one_floored(tmp_path):
    text, agg = _launch(tmp_path, "--free-bits", "0,0.05", "--latent-report")
    assert agg["failed_trials"] == [] and agg["free_bits"] == {"0": 0.0, "1": 0.05}
    assert list(agg) == DEFAULT_KEYS + ["free_bits", "latent"]
    assert "below_floor" in agg["latent"]["1"] and "below_floor" not in agg["latent"]["0"]
    assert 0 <= agg["latent"]["1"]["below_floor"] <= 20
    with open(tmp_path / "m" / "aggregate.json") as f:
        assert json.load(f)["free_bits"] == {"0": 0.0, "1": 0.05}
    e0, e1 = _epochs(tmp_path, 0), _epochs(tmp_path, 1)
    assert e0[0]["free_bits"] == 0.0 and abs(e1[0]["free_bits"] - 0.05) < 1e-8


def test_default_run_says_nothing_and_equals_a_zero_floor(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ta, agg = _launch(tmp_path / "a")
    assert list(agg) == DEFAULT_KEYS and "free_bits" not in ta
    with open(tmp_path / "a" / "m" / "aggregate.json") as f:
        assert list(json.load(f)) == DEFAULT_KEYS
    assert all("free_bits" not in r for r in _epochs(tmp_path / "a", 0))
    tb, aggb = _launch(tmp_path / "b", "--free-bits", "0")
    assert list(aggb) == DEFAULT_KEYS
    assert _stable(ta) == _stable(tb) and any("Test set loss" in l for l in _stable(ta))


def test_bad_floor_fails_before_any_epoch(tmp_path):
    rc, text = _launch(tmp_path, "--free-bits", "0.1,-1", rc_ok=False)
    assert rc != 0 and "free_bits must be finite and >= 0" in text
    assert "Train Epoch" not in text and "====> Epoch" not in text
