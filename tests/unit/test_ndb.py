"""NDB / JSD mode coverage (models/ndb.py) on the CPU: the statistics on hand-made counts, the oracle against the
cases' own loop, the domain, the torch backend through the command line, the flags and the aggregate."""
import importlib.util
import json
import math
import os
import re
import sys

import pytest
import torch

from multidisttorch_amd.launch import launch
from multidisttorch_amd.models import ndb
from tests import ndb_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _labels(real, fake):
    return torch.tensor([k for cs in (real, fake) for k, c in enumerate(cs) for _ in range(c)])


def test_stats_on_hand_made_counts():
    same = ndb.ndb_stats(_labels([10, 20, 0, 30], [20, 40, 0, 60]), 60, 4, 1.5, 2, 9)
    assert (same["ndb"], same["jsd"], same["missing"], same["ndb_over_k"]) == (0, 0.0, 0, 0.0)
    assert (same["K"], same["iters"], same["inertia"], same["moved"]) == (4, 9, 1.5, 2)
    s = ndb.ndb_stats(_labels([50, 50, 0], [100, 0, 0]), 100, 3)
    # both live bins differ (z = 50 / sqrt(0.75 * 0.25 * 0.02) = 8.2); the third is empty on both sides
    assert (s["ndb"], s["missing"], s["counts_real"], s["counts_fake"]) == (2, 1, [50, 50, 0], [100, 0, 0])
    # p = (1/2, 1/2), q = (1, 0), their mean (3/4, 1/4)
    assert s["jsd"] == pytest.approx(0.25 * math.log(2 / 3) + 0.25 * math.log(2) + 0.5 * math.log(4 / 3), rel=1e-12)


@pytest.mark.parametrize("case", nc.FIT)
def test_oracle_is_the_cases_loop_and_every_case_is_decided(case):
    c = nc.fit_case(*case)
    labels, mind, cent, moved, inertia = ndb.kmeans_rows(c["real"].double(), c["fake"].double(), case[4], nc.T_FIT, c["init"])
    assert torch.equal(labels, c["labels"]) and moved.tolist() == c["moved"] and moved[0] == case[1]
    assert float(inertia) == pytest.approx(c["inertia"], rel=1e-12)
    for shape in nc.ASSIGN[:4]:
        nc.assign_case(*shape)  # raises where the float64 oracle has a near tie


@pytest.mark.parametrize("args,text", [((1, 9, 5, 2, 5), "got 1 real rows"), ((9, 65537, 5, 2, 5), "got 65537 generated rows"),
                                       ((9, 9, 0, 2, 5), "got D = 0"), ((9, 9, 5, 1, 5), "got K = 1"),
                                       ((300, 9, 5, 257, 5), "got K = 257"), ((9, 9, 5, 10, 5), "K = 10 needs"),
                                       ((9, 9, 5, 2, 0), "got 0"), ((9, 9, 5, 2, 1001), "got 1001")])
def test_domain(args, text):
    with pytest.raises(ValueError, match=text):
        ndb.check_ndb_args(*args)
    ndb.check_ndb_args(256, 2, 65536, 256, 1000)


def _cli():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_ndb", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_needs_the_sample_pass_and_its_domain():
    mod = _cli()
    with pytest.raises(ValueError, match="needs --sample-report"):
        mod.parse_args(["--ndb", "8"])
    with pytest.raises(ValueError, match="NDB"):
        mod.parse_args(["--ndb", "65", "--sample-report", "64"])
    a = mod.parse_args(["--ndb", "8", "--sample-report", "64"])
    assert (a.ndb, a.ndb_iters) == (8, 20) and (mod.parse_args([]).ndb, mod.parse_args([]).ndb_iters) == (0, 20)


@pytest.mark.parametrize("flags", [["--ndb", "8"], []])
def test_torch_backend_run_prints_the_line_and_the_aggregate_carries_ndb_only_under_the_flag(flags, tmp_path):
    mdir = os.path.join(str(tmp_path), "m")
    cmd = [sys.executable, os.path.join(ROOT, "vae-hpo.py"), "--backend", "torch", "--synthetic", "--train-samples", "256",
           "--test-samples", "64", "--epochs", "1", "--ngroups", "1", "--no-results", "--metrics-dir", mdir,
           "--sample-report", "64"] + flags
    old = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        rc, outs = launch(cmd, 1, emulate="torchrun", timeout=300, capture=True,
                          extra_env={"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    finally:
        os.chdir(old)
    out = outs[0] or ""
    assert rc == 0, out[-4000:]
    agg = json.loads(re.search(r"MDT_AGGREGATE (.*)", out).group(1))
    with open(os.path.join(mdir, "aggregate.json")) as f:
        assert json.load(f) == agg
    if flags:
        assert re.search(r"====> Test set NDB-8: ndb \d+ \([0-9.]+\) JSD [0-9.]+ missing \d+ inertia \S+ moved \d+ \(20 iters\)$",
                         out, re.M), out[-2000:]
        assert list(agg)[-2:] == ["ndb", "best_trial_by_ndb_jsd"] and agg["best_trial_by_ndb_jsd"] == 0
        assert list(agg["ndb"]["0"]) == ["K", "iters", "ndb", "ndb_over_k", "jsd", "missing", "inertia", "moved"]
        assert (agg["ndb"]["0"]["K"], agg["ndb"]["0"]["iters"]) == (8, 20)
    else:
        assert "NDB" not in out and "ndb" not in agg and "best_trial_by_ndb_jsd" not in agg
