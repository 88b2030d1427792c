"""HPO trial specifications.

The reference's only per-trial knob is the epoch count: trial g trains
``epochs + g`` epochs with lr fixed at 1e-3 and beta = 1
(/root/reference/vae-hpo.py:202, :131, :58). ``TrialSpec`` keeps that default
and adds the (lr, beta) sweep the north star asks for.
"""

from __future__ import annotations

import math
from dataclasses import asdict, dataclass
from typing import List, Optional, Sequence

from . import objective
from .schedule import Schedule

__all__ = ["TrialSpec", "reference_schedule", "default_sweep", "parse_list", "build_specs"]


@dataclass(frozen=True)
class TrialSpec:
    group_id: int
    epochs: int
    lr: float = 1e-3
    beta: float = 1.0
    seed: int = 0
    # lr / KL-weight schedule (hpo/schedule.py), all off by default.
    # lr_decay_steps = 0 with cosine decay: the runner uses the trial's total step count
    lr_warmup_steps: int = 0
    lr_decay: str = "none"
    lr_decay_steps: int = 0
    lr_min_ratio: float = 0.0
    kl_anneal_steps: int = 0
    # the objective knobs, one field per row of hpo/objective.py (what each one is stands there), 0 = off
    free_bits: float = 0.0
    tc_weight: float = 0.0
    ema_decay: float = 0.0

    def to_dict(self):
        return asdict(self)

    def objective(self) -> dict:
        """The trial's objective knobs (hpo/objective.py) by name: the trainers' keyword arguments."""
        return {n: getattr(self, n) for n in objective.NAMES}

    def schedule(self, total_steps: Optional[int] = None) -> Schedule:
        """The trial's ``Schedule``; ``total_steps`` (epochs x batches per epoch)
        stands in for an unset ``lr_decay_steps`` under cosine decay."""
        T = self.lr_decay_steps
        if self.lr_decay == "cosine" and T == 0 and total_steps is not None:
            T = int(total_steps)
        return Schedule(self.lr_warmup_steps, self.lr_decay, T, self.lr_min_ratio, self.kl_anneal_steps)


def reference_schedule(num_groups: int, epochs: int, lr: float = 1e-3, beta: float = 1.0,
                       seed: int = 0) -> List[TrialSpec]:
    """Trial g: epochs + g epochs, same lr/beta (reference behaviour)."""
    return [TrialSpec(g, epochs + g, lr, beta, seed + g) for g in range(num_groups)]


def default_sweep(num_groups: int, epochs: int = 1, seed: int = 0) -> List[TrialSpec]:
    """A K-point (lr, beta) grid: lr log-spaced in [3e-4, 3e-3], beta in {0.5, 1, 2, 4}."""
    specs = []
    nb = 4 if num_groups >= 4 else max(1, num_groups)
    nl = math.ceil(num_groups / nb)
    for g in range(num_groups):
        li, bi = g // nb, g % nb
        lr = 3e-4 * (10 ** (li / max(1, nl - 1))) if nl > 1 else 1e-3
        beta = [1.0, 0.5, 2.0, 4.0][bi] if num_groups > 1 else 1.0
        specs.append(TrialSpec(g, epochs, float(lr), float(beta), seed + g))
    return specs


def parse_list(s: Optional[str], cast=float) -> Optional[List]:
    if s is None or s == "":
        return None
    return [cast(x) for x in str(s).split(",") if x.strip() != ""]


def build_specs(num_groups: int, epochs: int, lrs: Optional[Sequence[float]] = None,
                betas: Optional[Sequence[float]] = None, seed: int = 0,
                epoch_offset: bool = True, lr_warmups: Optional[Sequence[int]] = None,
                lr_decays: Optional[Sequence[str]] = None, lr_decay_steps: Optional[Sequence[int]] = None,
                lr_min_ratios: Optional[Sequence[float]] = None,
                kl_anneals: Optional[Sequence[int]] = None, **knobs) -> List[TrialSpec]:
    """Per-group specs. A single value broadcasts; a list is indexed by group (cycled).
    ``knobs``: the objective knobs of hpo/objective.py by name (``free_bits=``, ``tc_weight=``,
    ``ema_decay=``), each a scalar, a list or a comma list like ``--beta``, inside the knob's range."""
    def pick(vals, g, default):
        return vals[g % len(vals)] if vals else default

    for name, vals in knobs.items():
        if name not in objective.NAMES:
            raise TypeError(f"build_specs() got an unexpected keyword argument {name!r}")
        if vals is None or isinstance(vals, str):
            vals = parse_list(vals)
        elif isinstance(vals, (int, float)):
            vals = [vals]
        knobs[name] = [objective.check(name, v) for v in vals or []]
    out = []
    for g in range(num_groups):
        spec = TrialSpec(g, epochs + (g if epoch_offset else 0), float(pick(lrs, g, 1e-3)),
                         float(pick(betas, g, 1.0)), seed + g,
                         lr_warmup_steps=int(pick(lr_warmups, g, 0)), lr_decay=str(pick(lr_decays, g, "none")),
                         lr_decay_steps=int(pick(lr_decay_steps, g, 0)),
                         lr_min_ratio=float(pick(lr_min_ratios, g, 0.0)),
                         kl_anneal_steps=int(pick(kl_anneals, g, 0)),
                         **{name: pick(vals, g, 0.0) for name, vals in knobs.items()})
        # bad values fail here, not in the middle of a run (T = 0 under cosine is resolved by the runner)
        spec.schedule(total_steps=spec.lr_warmup_steps + 1 if spec.lr_decay_steps == 0 else None)
        out.append(spec)
    return out
