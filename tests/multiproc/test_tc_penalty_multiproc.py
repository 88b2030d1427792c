"""The total-correlation penalty over processes (gloo, torch backend): the
replicas of a group of 2 stay bitwise equal, ``vae-hpo.py --tc-weight 0,2``
trains trial 0 exactly as a run without the flag and trial 1 otherwise, the
metrics and the aggregate carry the fields, and a resume under another weight
fails."""
import json
import os
import re
import sys

import torch

from multidisttorch_amd.launch import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLI = os.path.join(ROOT, "vae-hpo.py")
WORKER = os.path.join(HERE, "tc_worker.py")
ENV = {"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "PYTHONPATH": ROOT}
COMMON = ["--ngroups", "2", "--epochs", "1", "--no-epoch-offset", "--backend", "torch", "--synthetic",
          "--train-samples", "256", "--test-samples", "128", "--batch-size", "64", "--no-results", "--metrics-dir", "m"]
DEFAULT_KEYS = ["metric", "trials", "samples", "wall_s", "value", "unit", "failed_trials"]


def _launch(cwd, *args, rc_ok=True):
    old = os.getcwd()
    os.chdir(str(cwd))
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


def _epochs(d, g):
    with open(d / "m" / f"trial-{g}.jsonl") as f:
        return [r for r in map(json.loads, f) if "epoch" in r]


def _weights(d, g):
    return torch.load(str(d / "ck" / f"trial-{g}" / "epoch-1.pt"), weights_only=True)


def test_replicas_of_a_group_stay_bitwise_equal():
    res = {}
    for w in ("2.0", "0.0"):
        rc, outs = launch([sys.executable, WORKER, w], 2, emulate="torchrun", timeout=180, extra_env=ENV, capture=True)
        text = "\n".join(o or "" for o in outs)
        assert rc == 0, text[-4000:]
        rs = [json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT ")]
        assert len(rs) == 2 and all(r["equal"] and r["step"] == 5 for r in rs), rs
        res[w] = rs[0]
    assert res["2.0"]["tc_weight"] == 2.0 and res["2.0"]["epoch_tc"] != 0.0
    assert res["0.0"]["tc_weight"] == 0.0 and res["0.0"]["epoch_tc"] == 0.0
    assert res["2.0"]["psum"] != res["0.0"]["psum"]  # the penalty entered the averaged gradients


def test_two_trials_one_penalised_and_resume(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    ta, agga = _launch(a, "--ckpt-dir", "ck")
    assert list(agga) == DEFAULT_KEYS and "tc_weight" not in ta
    assert all("train_tc" not in r and "tc_weight" not in r for r in _epochs(a, 0))
    tb, aggb = _launch(b, "--ckpt-dir", "ck", "--tc-weight", "0,2")
    assert aggb["failed_trials"] == [] and aggb["tc_weight"] == {"0": 0.0, "1": 2.0}
    assert list(aggb) == DEFAULT_KEYS + ["tc_weight"]
    with open(b / "m" / "aggregate.json") as f:
        assert json.load(f)["tc_weight"] == {"0": 0.0, "1": 2.0}
    # trial 0: the weights and metrics of the run without the flag
    ca, cb = _weights(a, 0), _weights(b, 0)
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    ea, eb = _epochs(a, 0)[0], _epochs(b, 0)[0]
    for k in ("train_loss_sum", "train_loss", "test_loss", "lr", "kl_beta"):
        assert ea[k] == eb[k], k
    assert eb["train_tc"] == 0.0 and eb["tc_weight"] == 0.0
    # trial 1 differs, and says how much total correlation it trained against
    c1a, c1b = _weights(a, 1), _weights(b, 1)
    assert any(not torch.equal(c1a["model"][k], c1b["model"][k]) for k in c1a["model"])
    e1 = _epochs(b, 1)[0]
    assert e1["tc_weight"] == 2.0 and e1["train_tc"] == e1["train_tc"] and e1["train_tc"] != 0.0
    assert c1b["objective"]["tc_weight"] == 2.0 and "tc_weight" not in cb["objective"]
    # a resume under another weight fails; under the same one it goes on
    rc, text = _launch(b, "--ckpt-dir", "ck", "--resume", "--epochs", "2", "--tc-weight", "0,3", rc_ok=False)
    assert "was trained with --tc-weight 2.0" in text
    text, agg = _launch(b, "--ckpt-dir", "ck", "--resume", "--epochs", "2", "--tc-weight", "0,2")
    assert "resumed trial 1" in text and agg["failed_trials"] == []


def test_bad_weight_fails_before_any_epoch(tmp_path):
    for bad in ("0.1,-1", "nan", "inf"):
        rc, text = _launch(tmp_path, "--tc-weight", bad, rc_ok=False)
        assert rc != 0 and "tc_weight must be finite and >= 0" in text
        assert "Train Epoch" not in text and "====> Epoch" not in text
