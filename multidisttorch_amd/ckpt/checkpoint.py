"""Per-trial checkpoint / resume (absent from the reference).

Layout (beside the reference's ``results-{group_rank}/`` images):

    <ckpt_dir>/trial-{g}/epoch-{e}.pt      one file per completed epoch
    <ckpt_dir>/trial-{g}/latest            text file: name of the newest epoch file

Each file holds only tensors and plain Python scalars/strings, so it loads
with ``torch.load(weights_only=True)`` (never unpickles code):
  model        state_dict under the reference's parameter names (fc1.weight, ...)
  optimizer    {"step", "exp_avg", "exp_avg_sq"} flat arenas (layout recorded), and
               "ema", the weight average, of a trainer that keeps one
  trial        TrialSpec fields (group_id, epochs, lr, beta, seed, and the
               lr / KL-weight schedule fields as given)
  schedule     the trainer's resolved Schedule (hpo/schedule.py) or None; a
               load restores it, so a resumed trial continues its schedule
               from the restored step
  progress     {"epoch": completed epochs, "step": optimizer steps}
  rng          {"seed", "rng_stream"} (Philox is counter-based: the step
               counter + seed fully determine the noise stream)
  layout       [[name, offset, shape...]] of the arena, for validation
  arch         model kind + dims (mlp: D/H/Z; conv: image/channels/Z + the
               layer table), validated on load before any tensor is copied
  data         {"binarize": none | threshold | static | dynamic}: the likelihood
               the trial trains under (data/binarize.py). ``load_latest`` returns
               it (absent = none); the runner refuses a resume under another one
  objective    the trainer's knobs of hpo/objective.py by name: the KL floor always, the
               penalty's weight and the decay of the weight average when > 0 (the average
               itself is ``optimizer.ema``); returned by ``load_latest`` (absent = 0) and
               checked by the runner in the same way
Only group rank 0 writes (replicas are identical after the all-reduce);
writes go to a temp file + atomic rename so a crash never leaves a torn file.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from ..hpo.objective import KNOBS

__all__ = ["trial_dir", "save_trial", "load_latest", "latest_path"]


def trial_dir(ckpt_dir: str, group_id: int) -> str:
    return os.path.join(ckpt_dir, f"trial-{group_id}")


def save_trial(ckpt_dir: str, trainer, spec, epoch: int, extra: Optional[dict] = None,
               binarize: str = "none") -> str:
    d = trial_dir(ckpt_dir, spec.group_id)
    os.makedirs(d, exist_ok=True)
    opt = trainer.optimizer_state()
    sched = getattr(trainer, "schedule", None)
    payload = {
        "format": "multidisttorch_amd.trial.v1",
        "model": trainer.state_dict(),
        "optimizer": {"step": int(opt["step"]), "exp_avg": opt["exp_avg"], "exp_avg_sq": opt["exp_avg_sq"]},
        "trial": {k: (float(v) if isinstance(v, float) else v if isinstance(v, str) else int(v))
                  for k, v in spec.to_dict().items()},
        "schedule": sched.to_dict() if sched is not None else None,
        "progress": {"epoch": int(epoch), "step": int(opt["step"])},
        "rng": {"seed": int(trainer.seed), "rng_stream": int(trainer.rng_stream)},
        "layout": [[n, int(o)] + [int(x) for x in s] for n, o, s in trainer.layout],
        "arch": trainer.model_meta(),
        "data": {"binarize": str(binarize)},
        "objective": {k.name: float(trainer.hp.get(k.name, 0.0)) for k in KNOBS
                      if k.always_saved or float(trainer.hp.get(k.name, 0.0)) > 0},
    }
    if opt.get("ema") is not None:
        payload["optimizer"]["ema"] = opt["ema"]
    if extra:
        payload["extra"] = extra
    name = f"epoch-{epoch}.pt"
    path = os.path.join(d, name)
    tmp = path + ".tmp"
    torch.save(payload, tmp)
    os.replace(tmp, path)
    with open(os.path.join(d, "latest.tmp"), "w") as f:
        f.write(name + "\n")
    os.replace(os.path.join(d, "latest.tmp"), os.path.join(d, "latest"))
    return path


def latest_path(ckpt_dir: str, group_id: int) -> Optional[str]:
    d = trial_dir(ckpt_dir, group_id)
    p = os.path.join(d, "latest")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        name = f.read().strip()
    path = os.path.join(d, name)
    return path if os.path.exists(path) else None


def load_latest(ckpt_dir: str, group_id: int, trainer) -> Optional[dict]:
    """Restore model + optimizer into ``trainer``; returns the progress dict or None."""
    path = latest_path(ckpt_dir, group_id)
    if path is None:
        return None
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if ck.get("format") != "multidisttorch_amd.trial.v1":
        raise ValueError(f"{path}: unknown checkpoint format {ck.get('format')!r}")
    arch = ck.get("arch")
    if arch is not None and arch != trainer.model_meta():
        raise ValueError(f"{path}: checkpoint is for {arch.get('kind')} model {arch}, "
                         f"trainer is {trainer.model_meta()}")
    lay = [[n, int(o)] + [int(x) for x in s] for n, o, s in trainer.layout]
    if ck["layout"] != lay:
        raise ValueError(f"{path}: parameter arena layout mismatch")
    trainer.load_state_dict(ck["model"])
    if ck.get("schedule") is not None:
        from ..hpo.schedule import Schedule

        trainer.set_schedule(Schedule(**ck["schedule"]))
    trainer.load_optimizer_state(ck["optimizer"])  # sets the step: the schedule continues from it
    return dict(ck["progress"], path=path, trial=ck["trial"], binarize=(ck.get("data") or {}).get("binarize", "none"),
                **{k.name: float((ck.get("objective") or {}).get(k.name, 0.0)) for k in KNOBS})
