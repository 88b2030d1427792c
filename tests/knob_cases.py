"""The combined configuration of the objective knobs, shared by
tests/unit/test_knob_cases.py, the f32 emulations of tests/unit/test_mlp_checker.py
and tests/unit/test_layer_checker.py, and tests/gpu/test_knob_combinations.py:
lr warm-up and cosine decay, KL annealing, a free-bits floor, the
total-correlation penalty, weight averaging, binarized rows and both Adam
options, all in force in the same step.

``ALL`` is the one table. The checked steps t = 5 and 6 (``STEP0 = 4``) sit on
the lr warm-up (W = 8) and on the KL ramp (A = 16), so the effective values are

    lr_t = lr t / 8          kl_t = float32(0.5 t / 16)
    tc_t = float32(float32(3.0) t / 16)
    1 - d_t = 1 - (1 + t) / (10 + t)   (the ramp of the average, below its cap 0.9)

and ``check_conditions`` asserts that each lies strictly inside its ramp: a
kernel that ignores a ramp computes another number.

Two stages live here because they are the same for every trainer (flat arenas):

  AD  ``conv_small_checker.adam_ref`` at ``adam_consts(adam, t)``: lr_t from the
      schedule, in the decoupled decay too, ``grad_scale`` on the gradient;
      params, exp_avg and exp_avg_sq within its derived bounds, w16 (conv) the
      bitwise bf16 twin of params.
  EM  ``ema_cases.oracle(e_before, params_after, decay, t)`` within
      ``ema_cases.bound`` (16 times the float32 oracle's own error).

The total-correlation share of d[mu|lv] (``tc_rule``): the existing reference
and bound of the reparameterisation backward, plus ``tc_t g64`` within
``tc_t bg + 2 u max(|before|, |after|)``, with ``g64`` / ``bg`` from
``tc_cases.bounds`` on the stored float32 mulv and eps (the float64 oracle of
models/latent.py and 16 times the float32 oracle's error). No number here comes
from a kernel.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from multidisttorch_amd.hpo.schedule import Schedule
from tests import conv_small_checker as sk
from tests import ema_cases as ec
from tests import tc_cases as tcc
from tests.igemm_checker import twin_ok
from tests.mlp_checker import U, ratio

SCHEDULE = Schedule(lr_warmup_steps=8, lr_decay="cosine", lr_decay_steps=32, lr_min_ratio=0.1, kl_anneal_steps=16)
KL_BETA, TC_WEIGHT, EMA_DECAY, LR = 0.5, 3.0, 0.9, 2e-3


def _adam_set(name):
    s = sk.ADAM_SETS[name]
    return dict(weight_decay=s["weight_decay"], decoupled_wd=s["decoupled"], grad_scale=s["grad_scale"])


ADAM = {"decoupled": _adam_set("decoupled"), "coupled": _adam_set("coupled")}
ALL = dict(schedule=SCHEDULE, kl_beta=KL_BETA, tc_weight=TC_WEIGHT, ema_decay=EMA_DECAY, lr=LR, adam=ADAM)

STEP0, CURSOR0 = 4, 1      # the state before the first checked step
STEPS = (5, 6)             # the checked optimizer steps t
HEAD_SCALE = 4.0           # tests/gpu/test_tc_penalty_gpu.py: the posteriors of an untrained encoder barely differ
MLP_SCALE = 6.0
SHARE, VISIBLE = 0.9, 4.0  # the visible-addend condition: this share of the floored elements, this many tolerances
TORCH_OMB = (sk.f32(1.0 - 0.9), sk.f32(1.0 - 0.999))  # the MLP kernels' moment weights (adam_common.h, torch_omb)


def trainer_kwargs(adam: str, tc: bool = True, fb: float = 0.0) -> dict:
    """Constructor keywords of either trainer for ALL with one Adam set;
    ``grad_scale`` is not one of them: ``apply`` sets it."""
    a = ADAM[adam]
    return dict(lr=LR, kl_beta=KL_BETA, schedule=SCHEDULE, free_bits=fb, tc_weight=TC_WEIGHT if tc else 0.0,
                ema_decay=EMA_DECAY, weight_decay=a["weight_decay"], decoupled_wd=a["decoupled_wd"])


def apply(tr, adam: str):
    tr.set_hparams(grad_scale=ADAM[adam]["grad_scale"])
    return tr


def effective(t: int, tc: bool = True, fb: float = 0.0) -> dict:
    """What ``read_state()`` must report after optimizer step t."""
    f = SCHEDULE.kl_factor(t)
    return dict(lr=LR * SCHEDULE.lr_factor(t), kl_beta=sk.f32(KL_BETA * f),
                tc_weight=sk.f32(float(np.float32(TC_WEIGHT)) * f) if tc else 0.0, free_bits=sk.f32(fb))


def check_conditions(t: int):
    """Strictly inside both ramps, and the average not yet at its cap."""
    e = effective(t)
    assert 0 < e["kl_beta"] < KL_BETA and 0 < e["lr"] < LR and 0 < e["tc_weight"] < TC_WEIGHT, (t, e)
    assert e["lr"] == LR * (t / 8) and e["kl_beta"] == sk.f32(0.5 * t / 16), (t, e)
    assert e["tc_weight"] == sk.f32(sk.f32(3.0) * t / 16), (t, e)
    assert (1.0 + t) / (10.0 + t) < EMA_DECAY and 1.0 - ec.d_t(EMA_DECAY, t) != 1.0 - EMA_DECAY, t


def assert_state(rs: dict, t: int, tc: bool = True, fb: float = 0.0):
    check_conditions(t)
    want = effective(t, tc, fb)
    got = {k: rs[k] for k in want}
    assert rs["step"] == t and got == want, (rs, want)


def adam_hp(adam: str) -> dict:
    """The hyper-parameter dict ``conv_small_checker.adam_consts`` / ``layer_checker.check_adam`` take (they
    evaluate the warm-up only: enough for t <= W, which ``adam_consts`` below asserts)."""
    a = ADAM[adam]
    return dict(lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=a["weight_decay"], grad_scale=a["grad_scale"],
                decoupled=a["decoupled_wd"], lr_warmup_steps=SCHEDULE.lr_warmup_steps)


def adam_consts(adam: str, t: int, omb=None) -> dict:
    """``conv_small_checker.adam_consts`` for ALL at optimizer step t, with lr_t of the whole schedule."""
    c = sk.adam_consts(adam_hp(adam), t, omb)
    lr_t = LR * SCHEDULE.lr_factor(t)
    assert c["lr"] == lr_t or t > SCHEDULE.lr_warmup_steps
    c["lr"], c["step_size"] = lr_t, lr_t / (1.0 - math.pow(0.9, t))
    return c


# ------------------------------------------------------------------- inputs ----
def binarize(X: torch.Tensor, seed: int = 13) -> torch.Tensor:
    """The Bernoulli resampling of grey rows (the ``bin`` kind of the case tables) for rows of any width."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(X.shape, generator=g) < X).float()


def _named_mask(tr):
    used = torch.zeros(tr.numel, dtype=torch.bool)
    for _, o, s in tr.layout:
        used[o: o + math.prod(s)] = True
    return used


def plant_optimizer_state(tr, seed: int = 11):
    """Adam moments as earlier steps could have left them (v >= m^2) and an average away from the parameters, on
    the named tensors only (padding stays zero)."""
    g = torch.Generator().manual_seed(seed)
    used = _named_mask(tr)
    m0 = (torch.rand(tr.numel, generator=g) - 0.5) * 1e-2
    v0 = m0 ** 2 + torch.rand(tr.numel, generator=g) * 1e-4
    rel = 1.0 + 0.05 * torch.randn(tr.numel, generator=g)
    dev = tr.params.device
    with torch.no_grad():
        tr.exp_avg.copy_((m0 * used).to(dev))
        tr.exp_avg_sq.copy_((v0 * used).to(dev))
        if tr.ema is not None:
            tr.ema.copy_(tr.params * (rel * used).to(dev))


# -------------------------------------------------------------------- rules ----
def tc_of(mulv, eps, tc_t: float):
    """The ``tc`` argument of the checkers' ``check_backward``: (tc_t, g64, bg), and (value64, value bound)."""
    v64, g64, bv, bg = tcc.bounds(mulv.detach().float().cpu(), eps.detach().float().cpu())
    return (float(tc_t), g64, bg), (v64, bv)


def tc_rule(ref, bound, tc):
    """(ref, bound) of d[mu|lv] with the penalty's share folded in; ``tc`` None: unchanged."""
    if tc is None:
        return ref, bound
    tc_t, g64, bg = tc
    add = tc_t * g64.to(ref.device)
    after = ref + add
    return after, bound + tc_t * bg + 2 * U * torch.maximum(ref.abs(), after.abs())


def visible_share(ref_bound_with, tc, floored) -> dict:
    """Share of the floored elements of each half (mu, lv) whose addend exceeds VISIBLE tolerances."""
    _, bound = ref_bound_with
    tc_t, g64, _ = tc
    Z = floored.shape[1]
    big = (tc_t * g64.to(bound.device)).abs() > VISIBLE * bound
    out = {}
    for name, sl in (("mu", slice(0, Z)), ("lv", slice(Z, 2 * Z))):
        f = floored.to(bound.device)
        out[name] = float(big[:, sl][f].double().mean()) if bool(f.any()) else 0.0
    return out


def assert_visible(ref_bound_with, tc, floored, label=""):
    share = visible_share(ref_bound_with, tc, floored)
    print(f"visible addend on the floored set {label}: mu {share['mu']:.3f} lv {share['lv']:.3f} (need {SHARE})")
    assert min(share.values()) >= SHARE, share


# ------------------------------------------------------------------- stages ----
def check_adam(before: dict, after: dict, grads, c: dict) -> dict:
    """``before`` / ``after``: dict(params, exp_avg, exp_avg_sq[, w16]) of flat arenas around the step;
    ``grads``: the gradient arena Adam consumed; ``c``: ``adam_consts``."""
    cpu = lambda t: t.detach().reshape(-1).cpu()
    rp, rm, rv, bp, bm, bv = sk.adam_ref(cpu(before["params"]), cpu(grads), cpu(before["exp_avg"]),
                                         cpu(before["exp_avg_sq"]), c)
    out = {"AD.params": ratio(cpu(after["params"]), rp, bp), "AD.exp_avg": ratio(cpu(after["exp_avg"]), rm, bm),
           "AD.exp_avg_sq": ratio(cpu(after["exp_avg_sq"]), rv, bv)}
    if after.get("w16") is not None:
        out["AD.w16"] = 0.0 if twin_ok(cpu(after["w16"]), cpu(after["params"])) else math.inf
    return out


def check_ema(e_before, params_after, ema_after, t: int, decay: float = EMA_DECAY) -> dict:
    e64, b = ec.bound(e_before, params_after, decay, t)
    err = (ema_after.detach().cpu().double() - e64).abs()
    if not bool(torch.isfinite(err).all()):
        return {"EM.ema": math.inf}
    return {"EM.ema": float(err.max()) / b}


# ------------------------------------------------- inputs of the three paths ----
MLP_SEED, CONV_SEED = 3, 2
MLP_NBATCH = 2
# (shape id of mlp_checker.SHAPES, rows M): the smallest shapes that reach the MLP kernels' paths
MLP_CASES = (("tiny", 16), ("tiny", 5), ("ragged", 37))


def mlp_data(sid: str):
    """(X [2 B + 7, D] binarized rows, idx [2 B]) on the CPU."""
    from tests.mlp_checker import SHAPES

    s = SHAPES[sid]
    g = torch.Generator().manual_seed(MLP_SEED)
    n = MLP_NBATCH * s["B"] + 7
    X = binarize(torch.rand(n, s["D"], generator=g))
    idx = torch.randperm(n, generator=g)[: MLP_NBATCH * s["B"]].to(torch.int32)
    return X, idx


def scale_mlp_heads(named: dict):
    with torch.no_grad():
        named["fc21.weight"].mul_(MLP_SCALE)
        named["fc22.weight"].mul_(MLP_SCALE)


def cursor_of(t: int, nbatches: int) -> int:
    """The cursor the state holds before optimizer step t."""
    return (CURSOR0 + t - STEPS[0]) % nbatches


def conv_params(init: dict, spec) -> dict:
    """The ``spread`` parameters of layer_checker (dead ReLUs, both BCE branches, nonzero biases) with the
    encoder head scaled by HEAD_SCALE over its initial values, as tests/gpu/test_tc_penalty_gpu.py does, so
    that the posteriors differ and the penalty's gradient is visible."""
    from tests.layer_checker import spread_params

    out = spread_params(init, spec)
    out["enc_head.weight"] = (init["enc_head.weight"].detach().float().cpu() * HEAD_SCALE).float()
    return out
