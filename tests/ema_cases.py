"""Shared inputs, oracle and bounds of the weight-averaging tests
(tests/unit/test_ema.py, tests/gpu/test_ema_gpu.py, tests/multiproc/test_ema_multiproc.py).

The oracle is the definition of docs/KERNELS.md, "Weight averaging", evaluated
in float64 on the float32 inputs: after optimizer step t (1-based)

    d_t = min(decay, (1 + t) / (10 + t))
    e  <-  e + (1 - d_t) * (p - e)

The bound follows tests/tc_cases.py: ``MARGIN`` = 16 times the error of the same
oracle run in float32 against the float64 one on the same inputs, floored by one
float32 rounding of the largest ``|p|`` or ``|e|`` that enters. It never comes
from the code under test. A chain of steps sums the steps' bounds: an error of
the average that enters a step leaves it multiplied by ``d_t < 1``.
"""
import torch

MARGIN = 16.0
U32 = 2.0 ** -24  # unit roundoff of float32

# the kernel-level sizes: the scalar tail alone, exactly one float4, one more element, 255 / 256 / 257,
# a ragged several-block size, 2^20 + 1 (1024 full blocks and a tail element) and, past the launch's
# cap of 2048 blocks x 256 lanes x 4 floats = 2^21 floats, a size whose second grid stride is ragged
KERNEL_NS = (1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 20 + 1, 2 ** 21 + 1029)
DECAYS = (0.9, 0.999)
# for decay 0.9 the ramp (1 + t) / (10 + t) meets the decay at t = 80
TS = (1, 79, 80, 81, 10 ** 6)
PAD = 8          # elements past n that must stay untouched
SENTINEL = -7.25

_worst = {"ratio": 0.0, "what": ""}


def d_t(decay: float, t: int) -> float:
    return min(float(decay), (1.0 + t) / (10.0 + t))


def inputs(n: int, seed: int = 5):
    """(e, p) float32: magnitudes from 1e-8 to 1e3, both signs, independent."""
    g = torch.Generator().manual_seed(seed + 7919 * (n % 1009))

    def one():
        mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 11.0 - 8.0)
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
        return (mag * sign).float()

    return one(), one()


def oracle(e, p, decay: float, t: int, dtype=torch.float64):
    """The average after optimizer step t from float32 ``e`` and ``p``, in ``dtype``."""
    e, p = e.detach().cpu().to(dtype), p.detach().cpu().to(dtype)
    omd = torch.tensor(1.0 - d_t(decay, t), dtype=torch.float64).to(dtype)
    return (e + omd * (p - e)).double()


def bound(e, p, decay: float, t: int):
    """(e64, bound) of one update."""
    e64 = oracle(e, p, decay, t)
    e32 = oracle(e, p, decay, t, torch.float32)
    scale = max(float(e.detach().abs().max()), float(p.detach().abs().max()))
    return e64, MARGIN * max(float((e32 - e64).abs().max()), U32 * scale)


def check(what: str, got, e64, b: float) -> float:
    """Prints the achieved error next to its bound, asserts, and keeps the worst ratio."""
    err = float((got.detach().cpu().double() - e64).abs().max())
    ratio = err / b if b > 0 else (0.0 if err == 0 else float("inf"))
    print(f"ema {what}: err {err:.3g} / bound {b:.3g} (ratio {ratio:.3g})")
    if ratio > _worst["ratio"]:
        _worst["ratio"], _worst["what"] = ratio, what
    assert err <= b, (what, err, b)
    return ratio


def worst():
    return dict(_worst)


def check_chain(what: str, e0, params_after, averages_after, decay, t0: int = 0):
    """A run of steps t0 + 1 ..: ``params_after[k]`` / ``averages_after[k]`` are
    the float32 arenas after step t0 + k + 1, ``e0`` the average before.

    Every step against the one-step oracle from the average the code itself held
    before it, and the whole chain against the float64 chain from ``e0`` under
    the sum of the steps' bounds."""
    prev = e0.detach().cpu()
    chain = prev.double()
    total = 0.0
    for k, (p, e) in enumerate(zip(params_after, averages_after)):
        t = t0 + k + 1
        e64, b = bound(prev, p, decay, t)
        check(f"{what} step {t}", e, e64, b)
        omd = 1.0 - d_t(decay, t)
        chain = chain + omd * (p.detach().cpu().double() - chain)
        total += b
        check(f"{what} chain to step {t}", e, chain, total)
        prev = e.detach().cpu()
