"""Weight averaging over processes (gloo, torch backend): the replicas of a group
of 2 hold bitwise equal averages, ``vae-hpo.py --ema-decay 0,0.99`` keeps the
stdout format, trains trial 0 exactly as a run without the flag, scores trial 1
under its average, puts ``ema_decay`` and ``test_loss_raw`` into the aggregate,
and a resume under another decay fails."""
import json
import os
import re
import sys

import torch

from multidisttorch_amd.launch import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLI = os.path.join(ROOT, "vae-hpo.py")
WORKER = os.path.join(HERE, "ema_worker.py")
ENV = {"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "PYTHONPATH": ROOT}
COMMON = ["--ngroups", "2", "--epochs", "1", "--no-epoch-offset", "--backend", "torch", "--synthetic",
          "--train-samples", "256", "--test-samples", "128", "--batch-size", "64", "--no-results", "--metrics-dir", "m",
          "--lr", "3e-3"]
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
        return rc, text, outs
    assert rc == 0, text[-4000:]
    return text, json.loads(re.search(r"MDT_AGGREGATE (.*)", text).group(1)), outs


def _epochs(d, g):
    with open(d / "m" / f"trial-{g}.jsonl") as f:
        return [r for r in map(json.loads, f) if "epoch" in r]


def _ckpt(d, g, epoch=1):
    return torch.load(str(d / "ck" / f"trial-{g}" / f"epoch-{epoch}.pt"), weights_only=True)


def _stdout_lines(out):
    """A rank's output lines that do not vary from run to run: no wall-clock, aggregate or master-port
    line (nor c10d's timestamped log lines: the capture carries stderr too)."""
    return [l for l in (out or "").splitlines()
            if "Done. time:" not in l and not l.startswith("MDT_AGGREGATE") and " master at " not in l
            and not re.match(r"\[[WEI]\d{4} ", l)]


def _shape(lines):
    """The lines with every number replaced: the format alone."""
    return [re.sub(r"-?\d+(\.\d+)?(e-?\d+)?", "#", l) for l in lines]


def test_replicas_of_a_group_hold_bitwise_equal_averages():
    rc, outs = launch([sys.executable, WORKER, "0.9"], 2, emulate="torchrun", timeout=180, extra_env=ENV, capture=True)
    text = "\n".join(o or "" for o in outs)
    assert rc == 0, text[-4000:]
    rs = {r["rank"]: r for r in (json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT "))}
    assert sorted(rs) == [0, 1], text[-4000:]
    assert not rs[0]["stale_before_reset"] and rs[1]["stale_before_reset"]  # the reset after the broadcast matters
    for r in rs.values():
        assert r["params_equal"] and r["ema_equal"] and r["moved"] and r["step"] == 5, r


def test_two_trials_one_averaged_and_resume(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    ta, agga, outa = _launch(a, "--ckpt-dir", "ck")
    assert list(agga) == DEFAULT_KEYS and "ema_decay" not in ta and "test_loss_raw" not in ta
    assert all("ema_decay" not in r for r in _epochs(a, 0))
    assert "ema" not in _ckpt(a, 0)["optimizer"] and "ema_decay" not in _ckpt(a, 0)["objective"]
    tb, aggb, outb = _launch(b, "--ckpt-dir", "ck", "--ema-decay", "0,0.99")
    assert aggb["failed_trials"] == [] and aggb["ema_decay"] == {"0": 0.0, "1": 0.99}
    assert list(aggb) == DEFAULT_KEYS + ["ema_decay", "test_loss_raw"]
    with open(b / "m" / "aggregate.json") as f:
        assert json.load(f) == aggb
    # the stdout format is unchanged: rank 0 (trial 0, no average) prints what the run without the flag prints,
    # byte for byte; rank 1 (trial 1) prints lines of the same shape
    assert _stdout_lines(outa[0]) == _stdout_lines(outb[0]) and len(_stdout_lines(outa[0])) > 3
    assert _shape(_stdout_lines(outa[1])) == _shape(_stdout_lines(outb[1]))
    assert _stdout_lines(outa[1]) != _stdout_lines(outb[1])  # its test loss is the average's
    # trial 0: the weights and metrics of the run without the flag
    ca, cb = _ckpt(a, 0), _ckpt(b, 0)
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    ea, eb = _epochs(a, 0)[0], _epochs(b, 0)[0]
    for k in ("train_loss_sum", "train_loss", "test_loss", "lr", "kl_beta"):
        assert ea[k] == eb[k], k
    assert eb["ema_decay"] == 0.0 and "ema" not in cb["optimizer"] and "ema_decay" not in cb["objective"]
    # trial 1 trains the same raw weights, but every score is under the average
    c1a, c1b = _ckpt(a, 1), _ckpt(b, 1)
    for k in c1a["model"]:
        assert torch.equal(c1a["model"][k], c1b["model"][k]), k
    e1a, e1b = _epochs(a, 1)[0], _epochs(b, 1)[0]
    assert e1b["ema_decay"] == 0.99 and e1a["train_loss_sum"] == e1b["train_loss_sum"]
    assert e1a["test_loss"] != e1b["test_loss"]
    assert c1b["objective"]["ema_decay"] == 0.99 and c1b["optimizer"]["ema"].shape == c1b["optimizer"]["exp_avg"].shape
    assert not torch.equal(c1b["optimizer"]["ema"], c1b["optimizer"]["exp_avg"])
    # test_loss_raw: the raw weights' test loss. The run without the flag scored the same weights, in a pass
    # that drew other eval noise (the noise follows the eval state's step), so the two agree only closely
    assert list(aggb["test_loss_raw"]) == ["1"]
    raw = aggb["test_loss_raw"]["1"]
    print(f"trial 1 test loss: averaged {e1b['test_loss']:.4f} raw {raw:.4f} (run without the flag {e1a['test_loss']:.4f})")
    assert abs(raw - e1a["test_loss"]) <= 0.05 * abs(e1a["test_loss"]) and raw != round(e1b["test_loss"], 4)
    # a resume under another decay fails; under the same one it goes on
    rc, text, _ = _launch(b, "--ckpt-dir", "ck", "--resume", "--epochs", "2", "--ema-decay", "0,0.9", rc_ok=False)
    assert "was trained with --ema-decay 0.99, this run asks for --ema-decay 0.9" in text
    text, agg, _ = _launch(b, "--ckpt-dir", "ck", "--resume", "--epochs", "2", "--ema-decay", "0,0.99")
    assert "resumed trial 1" in text and agg["failed_trials"] == []
    assert not torch.equal(_ckpt(b, 1, 2)["optimizer"]["ema"], c1b["optimizer"]["ema"])


def test_bad_decay_fails_before_any_epoch(tmp_path):
    for bad in ("0.1,1", "-0.5", "nan"):
        rc, text, _ = _launch(tmp_path, "--ema-decay", bad, rc_ok=False)
        assert rc != 0 and "ema_decay must be" in text
        assert "Train Epoch" not in text and "====> Epoch" not in text
