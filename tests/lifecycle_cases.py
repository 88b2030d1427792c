"""One trial run twice, through ``run_trial`` and through ``run_packed_trials``
(one spec, ``num_trials=1``), in this process on data passed as ``data=``: the
two entry points share the trial lifecycle (resume, data binding, after-trial
passes), so everything but the ``(trial g) `` tag and the clock agrees. Used by
tests/unit/test_trial_lifecycle.py (torch backend) and tests/gpu/test_e2e_gpu.py
(hip backend)."""
import json
import os

import torch

from multidisttorch_amd.ckpt import checkpoint as ckpt
from multidisttorch_amd.data.datasets import ImageSet, synthetic_images
from multidisttorch_amd.hpo.runner import RunOptions, run_packed_trials, run_trial
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.runtime.bootstrap import bound_device

B, N_TRAIN, N_TEST = 16, 40, 24   # two full batches and a tail of 8; a test set of one batch and a tail of 8
KNOBS = dict(free_bits=0.05, tc_weight=0.5, ema_decay=0.9)


def _timeless(d):
    """``d`` without the clock: ``ts``, every ``*_s`` field and the rate derived from one."""
    if isinstance(d, dict):
        return {k: _timeless(v) for k, v in d.items()
                if not (k == "ts" or k.endswith("_s") or k == "train_samples_per_s")}
    return d


def run_both(model: str, backend: str, tmp_path):
    """-> {"single" | "packed": dict(result=TrialResult, extra=its extra without timings,
    events=the metrics JSONL without timings, ckpt=the epoch-1 checkpoint payload)}"""
    dev = bound_device()
    data = tuple(ImageSet(synthetic_images(n, seed=s), (1, 28, 28), True, "synthetic28").to(dev)
                 for n, s in ((N_TRAIN, 0), (N_TEST, 1)))
    spec = build_specs(1, 1, [3e-3], None, 5, **KNOBS)[0]
    out = {}
    for how in ("single", "packed"):
        d = os.path.join(str(tmp_path), f"{model}-{how}")
        opts = RunOptions(batch_size=B, backend=backend, model=model, results=False, ckpt_dir=os.path.join(d, "ck"),
                          metrics_dir=os.path.join(d, "m"), iw_samples=2, latent_report=True,
                          report_objective=tuple(KNOBS))
        if how == "single":
            res = run_trial(spec, None, opts, data=data, num_trials=1)
        else:
            (res,) = run_packed_trials([spec], None, opts, data=data, num_trials=1)
        with open(os.path.join(d, "m", "trial-0.jsonl")) as f:
            events = [_timeless(json.loads(line)) for line in f]
        out[how] = dict(result=res, extra=_timeless(res.extra), events=events,
                        ckpt=torch.load(ckpt.latest_path(os.path.join(d, "ck"), 0), weights_only=True))
    return out


def same_nested(a, b) -> bool:
    """Equal nested dicts / lists with bitwise-equal tensors."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(same_nested(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same_nested(x, y) for x, y in zip(a, b))
    return a == b
