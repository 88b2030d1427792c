"""Per-trial learning-rate and KL-weight schedules.

``t >= 1`` is the 1-based optimizer step (Adam's ``t``; ``TrainState.step``
once the step has been advanced). With W = ``lr_warmup_steps``, T =
``lr_decay_steps`` (total steps, warm-up included), r = ``lr_min_ratio`` and
A = ``kl_anneal_steps``::

    f_lr(t) = t / W                                  if W > 0 and t <= W
            = r + (1-r) * 0.5 * (1 + cos(pi * p)),   p = min(1, (t-W)/(T-W))   if lr_decay == "cosine"
            = 1                                      otherwise
    f_kl(t) = min(1, t / A) if A > 0 else 1

    lr_t   = lr * f_lr(t)                 (double)
    beta_t = float32(kl_beta * f_kl(t))   (training loss and KLD gradient of step t)

Evaluation always uses the full ``kl_beta``. The all-default schedule returns
exactly 1.0 from both factors, so ``lr * 1.0`` and ``float32(kl_beta)`` are
the unscheduled values bit for bit. The HIP kernels evaluate the same
arithmetic on the device from the step counter they advance
(``csrc/kernels/vae_mlp.h``: ``sched_lr_factor`` / ``sched_kl_factor``), so a
captured graph of many steps needs no host involvement; the torch backends
apply these functions per step.
"""

from __future__ import annotations

import math
from dataclasses import asdict, dataclass

__all__ = ["Schedule", "LR_DECAYS", "FIELDS"]

LR_DECAYS = ("none", "cosine")
FIELDS = ("lr_warmup_steps", "lr_decay", "lr_decay_steps", "lr_min_ratio", "kl_anneal_steps")
_MAX_STEPS = 2 ** 31 - 1  # the device keeps the step parameters as int32


def _steps(name: str, v) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    v = int(v)
    if not 0 <= v <= _MAX_STEPS:
        raise ValueError(f"{name} must be in [0, 2^31), got {v}")
    return v


@dataclass(frozen=True)
class Schedule:
    lr_warmup_steps: int = 0
    lr_decay: str = "none"
    lr_decay_steps: int = 0
    lr_min_ratio: float = 0.0
    kl_anneal_steps: int = 0

    def __post_init__(self):
        for name in ("lr_warmup_steps", "lr_decay_steps", "kl_anneal_steps"):
            object.__setattr__(self, name, _steps(name, getattr(self, name)))
        if self.lr_decay not in LR_DECAYS:
            raise ValueError(f"lr_decay must be one of {LR_DECAYS}, got {self.lr_decay!r}")
        r = float(self.lr_min_ratio)
        if not 0.0 <= r <= 1.0:  # also rejects NaN
            raise ValueError(f"lr_min_ratio must be in [0, 1], got {self.lr_min_ratio!r}")
        object.__setattr__(self, "lr_min_ratio", r)
        if self.lr_decay == "cosine" and self.lr_decay_steps <= self.lr_warmup_steps:
            raise ValueError(f"cosine decay needs lr_decay_steps > lr_warmup_steps "
                             f"(got {self.lr_decay_steps} <= {self.lr_warmup_steps})")

    @property
    def active(self) -> bool:
        """False when both factors are 1 at every step."""
        return bool(self.lr_warmup_steps or self.lr_decay != "none" or self.kl_anneal_steps)

    def lr_factor(self, t: int) -> float:
        W, T, r = self.lr_warmup_steps, self.lr_decay_steps, self.lr_min_ratio
        if W > 0 and t <= W:
            return t / W
        if self.lr_decay == "cosine":
            p = min(1.0, (t - W) / (T - W))
            return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * p))
        return 1.0

    def kl_factor(self, t: int) -> float:
        A = self.kl_anneal_steps
        return min(1.0, t / A) if A > 0 else 1.0

    def to_dict(self) -> dict:
        return asdict(self)

    def native_args(self) -> dict:
        """Keyword arguments of the native ``set_hparams`` (decay kind as its device code)."""
        return dict(lr_warmup_steps=self.lr_warmup_steps, lr_decay=LR_DECAYS.index(self.lr_decay),
                    lr_decay_steps=self.lr_decay_steps, lr_min_ratio=self.lr_min_ratio,
                    kl_anneal_steps=self.kl_anneal_steps)
