"""The per-trial objective knobs: one row each, read by everything above the kernels.

A knob is a float per trial (on the command line a scalar or a comma list) that
changes what the training step computes; 0 = off. Its name is the ``TrialSpec``
field, the ``trainer.hp`` key, the checkpoint's ``objective`` key and the
aggregate's key. vae-hpo.py, hpo/trial.py, hpo/runner.py, hpo/aggregate.py,
ckpt/checkpoint.py and models/trainer_base.py loop over ``KNOBS``; docs/KNOBS.md
lists what a new row leaves to do. This module imports nothing of the package.
"""

from __future__ import annotations

import math
from dataclasses import dataclass


@dataclass(frozen=True)
class Knob:
    name: str
    help: str           # of the command-line flag
    below_one: bool     # admissible: [0, 1) instead of every finite value >= 0
    always_saved: bool  # the checkpoint records the value always, not only when > 0 (absent = 0 either way)
    structural: bool    # a trainer built with 0 has no launches for it and refuses a positive value later

    @property
    def flag(self) -> str:
        return "--" + self.name.replace("_", "-")


KNOBS = (
    # free bits: KL floor in nats per sample and latent dimension (csrc/kernels/common.h)
    Knob("free_bits", "free bits: a floor in nats under each latent dimension's KL term of each sample "
         "(training objective only; 0 = off), comma list per trial", False, True, False),
    # total-correlation penalty: weight of the minibatch TC estimate in the objective (models/tc.py)
    Knob("tc_weight", "weight of the minibatch total-correlation penalty in the training objective "
         "(--beta 1 --tc-weight b-1 is beta-TCVAE; 0 = off), comma list per trial", False, False, True),
    # weight averaging: decay of the parameter average every evaluation uses (docs/KERNELS.md, "Weight averaging")
    Knob("ema_decay", "decay of an exponential moving average of the weights, in [0, 1); every evaluation "
         "(test loss, --iw-samples, --latent-report, samples) then uses the average "
         "(0 = off), comma list per trial", True, False, True),
)
NAMES = tuple(k.name for k in KNOBS)
BY_NAME = {k.name: k for k in KNOBS}


def check(name: str, v, built=None) -> float:
    """``v`` as a float inside the knob's range, or ValueError. ``built``: for a
    trainer that exists, the structural knobs it was constructed with."""
    v, knob = float(v), BY_NAME[name]
    if not (math.isfinite(v) and 0.0 <= v < (1.0 if knob.below_one else math.inf)):
        raise ValueError(f"{name} must be {'in [0, 1)' if knob.below_one else 'finite and >= 0'}, got {v}")
    if built is not None and knob.structural and v > 0 and name not in built:
        raise ValueError(f"{name} > 0 needs a trainer built with {name} > 0 (the step's launch list differs)")
    return v


def reported(specs) -> tuple:
    """The knobs some trial of the run sets: the metrics and the aggregate carry every trial's value of them."""
    return tuple(n for n in NAMES if any(getattr(s, n) > 0 for s in specs))
