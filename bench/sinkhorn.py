#!/usr/bin/env python3
"""Time the Sinkhorn divergence kernels (``C.sinkhorn_rows``, csrc/kernels/sinkhorn.hip).

At D = 784 and D = 16384: ``--rows`` real against ``--rows`` generated rows
(uniform random pixels: the kernels' time does not depend on the values), blur
``--blur``, ``--iters`` iterations, after a warm-up round; median and spread of
``--passes`` rounds. In the same process, alternated round by round:

  * ``sinkhorn_cost``: the cost phase alone (norms, the three matrices, m);
  * ``sinkhorn_step``: one iteration alone (both launches), ``--reps``
    back-to-back between two synchronisations, with the bytes of the three
    matrices over its time as ``step_gbps``;
  * ``sinkhorn_rows``: the whole call;
  * ``stock_cost``, ``stock_step``, ``stock_rows``: the baseline. The same result
    from stock float32 torch ops on the same device: ``torch.mm`` for the costs,
    ``torch.logsumexp`` over the stored matrices for every softmin.

The record also carries the largest difference between the two potentials'
tables and the statistics from each. Prints one JSON line per D (times in ms).
Nothing here is tuned: the baseline runs as it ships.

    python bench/sinkhorn.py [--D 784,16384] [--rows 10000] [--blur 0.05] [--iters 100] [--passes 5] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, dev, reps):
    import torch

    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3 / reps


def _stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "passes": len(v)}


def stock_cost(real, fake):
    """(Cxy, Cxx, Cyy, m) from stock torch ops (float32)."""
    import torch

    nx, ny = (real * real).sum(1), (fake * fake).sum(1)
    sq = lambda x, y, a, b: (a[:, None] + b[None] - 2.0 * torch.mm(x, y.t())).clamp_min_(0.0)
    Cxx, Cyy = sq(real, real, nx, nx).fill_diagonal_(0.0), sq(fake, fake, ny, ny).fill_diagonal_(0.0)
    return sq(real, fake, nx, ny), Cxx, Cyy, Cxx.mean()


def stock_step(costs, pots, eps, last):
    """One iteration on (f, g, p, q) from stock torch ops; -> the new potentials (the softmins when ``last``)."""
    import torch

    Cxy, Cxx, Cyy, _ = costs
    f, g, p, q = pots
    la, lb = -math.log(f.numel()), -math.log(g.numel())
    soft = lambda C, h, lw, dim: -eps * torch.logsumexp(lw + (h - C) / eps, dim=dim)
    new = (soft(Cxy, g[None, :], lb, 1), soft(Cxy, f[:, None], la, 0), soft(Cxx, p[None, :], la, 1), soft(Cyy, q[None, :], lb, 1))
    return new if last else tuple((a + b) / 2 for a, b in zip(pots, new))


def stock_rows(real, fake, E, T):
    import torch

    costs = stock_cost(real, fake)
    pots = tuple(torch.zeros(n, device=real.device) for n in (real.shape[0], fake.shape[0]) * 2)
    for t in range(T):
        eps = max(E, 4.0 * 0.5 ** t) * costs[3]
        old, pots = pots, stock_step(costs, pots, eps, t == T - 1)
    marg = (torch.exp((old[0] - pots[0]) / eps) - 1).abs().mean()
    return torch.stack([torch.cat(pots[:2]), torch.cat(pots[2:])], 1), costs[3], marg


def run(D: int, rows: int, E: float, T: int, passes: int, reps: int):
    import torch

    from multidisttorch_amd.models import sinkhorn as sk
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(D)
    real, fake = (torch.rand(rows, D, generator=g).to(dev) for _ in range(2))
    ws = torch.empty(C.sinkhorn_ws_numel(rows, rows), dtype=torch.float32, device=dev)
    pot = torch.empty(2 * rows, sk.COLS, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    res = {"costs": stock_cost(real, fake)}
    res["pots"] = tuple(torch.zeros(rows, device=dev) for _ in range(4))
    mid = T // 2   # an iteration past the anneal's start; neither side's time depends on the values
    eps_mid = max(E, 4.0 * 0.5 ** mid) * res["costs"][3]
    fns = {
        "sinkhorn_cost": (lambda: C.sinkhorn_cost(real, fake, ws), reps),
        "sinkhorn_step": (lambda: C.sinkhorn_step(rows, rows, E, T, mid, ws, pot, out), reps),
        "sinkhorn_rows": (lambda: C.sinkhorn_rows(real, fake, E, T, ws, pot, out), 1),
        "stock_cost": (lambda: res.__setitem__("costs", stock_cost(real, fake)), reps),
        "stock_step": (lambda: res.__setitem__("pots", stock_step(res["costs"], res["pots"], eps_mid, False)), reps),
        "stock_rows": (lambda: res.__setitem__("stock", stock_rows(real, fake, E, T)), 1),
    }
    for f, _ in fns.values():  # warm-up: code objects, GEMM algorithm choice, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, (f, n) in fns.items():
            times[k].append(_timed(f, dev, n))
    C.sinkhorn_rows(real, fake, E, T, ws, pot, out)   # the timed steps advanced the workspace: the result afresh
    torch.cuda.synchronize(dev)
    keys = ("scale", "sinkhorn", "w2", "ot", "marg_err")
    ours = sk.sinkhorn_stats(pot, rows, out[0], out[1], E, T)
    stock = sk.sinkhorn_stats(res["stock"][0], rows, res["stock"][1], res["stock"][2], E, T)
    step_bytes = 4.0 * 3 * rows * rows
    rec = {"rows": rows, "D": D, "blur": E, "iters": T, "reps": reps, "kernels": {k: float(f"{ours[k]:.7g}") for k in keys},
           "stock": {k: float(f"{stock[k]:.7g}") for k in keys},
           "max_abs_diff_pot": float((pot - res["stock"][0]).abs().max()),
           "cost_flop": 2.0 * 2 * rows * rows * D, "step_bytes": step_bytes}
    for k, v in times.items():
        rec[k] = _stats(v)
    rec["cost_tflops"] = round(rec["cost_flop"] / (rec["sinkhorn_cost"]["median_ms"] * 1e-3) / 1e12, 1)
    rec["step_gbps"] = round(step_bytes / (rec["sinkhorn_step"]["median_ms"] * 1e-3) / 1e9, 1)
    for part in ("cost", "step", "rows"):
        rec[f"stock_over_kernels_{part}"] = round(rec[f"stock_{part}"]["median_ms"] / rec[f"sinkhorn_{part}"]["median_ms"], 2)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", default="784,16384")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--blur", type=float, default=0.05)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/sinkhorn.py measures the HIP backend: no GPU found")
    recs = []
    for D in a.D.split(","):
        r = run(int(D), a.rows, a.blur, a.iters, max(5, a.passes), max(1, a.reps))
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
