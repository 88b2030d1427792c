"""``vae-hpo.py --binarize dynamic`` on a group of two (gloo, torch backend):
the draws are keyed by the trial seed and the global data-set row, so the
replicas binarize alike without communicating and stay bitwise in sync; the
aggregate line names the likelihood. A default run says nothing about it."""
import json
import os
import re
import sys

from multidisttorch_amd.launch import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "binarize_worker.py")
ENV = {"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "PYTHONPATH": ROOT}
COMMON = ["--ngroups", "1", "--epochs", "2", "--backend", "torch", "--synthetic", "--train-samples", "512",
          "--test-samples", "256", "--batch-size", "64", "--no-results", "--metrics-dir", "m"]
# the aggregate keys of a run without extensions
DEFAULT_KEYS = ["metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials"]


def _launch(tmp_path, *args):
    old = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        rc, outs = launch([sys.executable, WORKER] + COMMON + list(args), 2, emulate="torchrun", timeout=300,
                          extra_env=ENV, capture=True)
    finally:
        os.chdir(old)
    text = "\n".join(o or "" for o in outs)
    assert rc == 0, text[-4000:]
    res = [json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT ")]
    agg = json.loads(re.search(r"MDT_AGGREGATE (.*)", text).group(1))
    return text, res, agg


def test_replicas_binarize_alike_and_the_aggregate_names_the_mode(tmp_path):
    text, res, agg = _launch(tmp_path, "--binarize", "dynamic")
    assert sorted(r["rank"] for r in res) == [0, 1]
    # 512 rows in batches of 64: 8 steps per epoch on every replica
    assert res[0]["step"] == res[1]["step"] == 16
    assert res[0]["digest"] == res[1]["digest"]
    assert agg["binarize"] == "dynamic" and agg["failed_trials"] == []
    assert list(agg) == DEFAULT_KEYS + ["binarize"]
    with open(tmp_path / "m" / "aggregate.json") as f:
        assert json.load(f)["binarize"] == "dynamic"
    assert re.search(r"^\[0:0\] ====> Test set loss: \d+\.\d{4}$", text, re.M)


def test_default_run_carries_no_binarize_key(tmp_path):
    text, res, agg = _launch(tmp_path)
    assert res[0]["digest"] == res[1]["digest"]
    assert list(agg) == DEFAULT_KEYS
    assert "binarize" not in text
    with open(tmp_path / "m" / "aggregate.json") as f:
        assert list(json.load(f)) == DEFAULT_KEYS
