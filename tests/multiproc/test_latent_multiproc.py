"""``--latent-report`` on a group of two (gloo, torch backend): the pass keys
its noise by the trial seed alone, so both replicas report the same numbers."""
import json
import math
import os
import sys

import pytest

from multidisttorch_amd.launch import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "latent_worker.py")
ENV = {"DDP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "PYTHONPATH": ROOT}


@pytest.mark.parametrize("model", ["mlp", "conv"])
def test_both_members_report_identical_numbers(tmp_path, model):
    old = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        rc, outs = launch([sys.executable, WORKER, model], 2, emulate="torchrun", timeout=300, extra_env=ENV,
                          capture=True)
    finally:
        os.chdir(old)
    text = "\n".join(o or "" for o in outs)
    assert rc == 0, text[-4000:]
    res = [json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT ")]
    assert sorted(r["rank"] for r in res) == [0, 1] and sorted(r["grank"] for r in res) == [0, 1], text[-2000:]
    a, b = res
    assert not a["failed"] and not b["failed"]
    assert a["latent"] == b["latent"]
    lat = a["latent"]
    assert lat["rows"] == 85 and lat["kl"] > 0 and 0 <= lat["mi"] <= math.log(85) + 1e-3
    assert abs(lat["mi"] + lat["tc"] + lat["dwkl"] - lat["sampled_kl"]) < 1e-4
    # the group leader prints the line once
    assert text.count("====> Test set latent: KL") == 1
