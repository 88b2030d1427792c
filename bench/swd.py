#!/usr/bin/env python3
"""Time the sliced Wasserstein kernels (``C.swd_rows``, csrc/kernels/swd.hip).

At D = 784 and D = 16384: ``--rows`` real against ``--rows`` generated rows
(uniform random pixels: the kernels' time does not depend on the values; the
sort is a fixed network), ``--dirs`` directions from ``swd_directions``, after a
warm-up round; median and spread of ``--passes`` rounds, each round timing
``--reps`` back-to-back calls between two synchronisations (a single call is
well under a millisecond at D = 784) and reporting the time per call. In the
same process, alternated round by round:

  * ``swd_project`` and ``swd_sort``: the two launches alone (the second on the
    first's output; a sorted input costs the network the same);
  * ``swd_rows``: the whole call, both launches;
  * ``stock_torch``: the baseline. The same table from stock float32 torch ops on
    the same device: ``torch.mm``, ``torch.sort``, the segment means by indexing.

The record also carries the largest difference between the two results and the
statistics from each. Prints one JSON line per D (times in ms). Nothing here is
tuned: the baseline runs as it ships.

    python bench/swd.py [--D 784,16384] [--rows 10000] [--dirs 512] [--passes 7] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
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


def stock_rows(real, fake, dirs, seg):
    """(proj, table) from stock torch ops (float32)."""
    import torch

    na, nb = real.shape[0], fake.shape[0]
    sr, sf = torch.mm(dirs, real.t()).sort(1).values, torch.mm(dirs, fake.t()).sort(1).values
    i, j, w = seg
    d = sr[:, i] - sf[:, j]
    return torch.cat([sr, sf], 1), torch.stack([(d.abs() * w).sum(1), (d * d * w).sum(1)], 1) / float(na * nb)


def run(D: int, rows: int, P: int, passes: int, reps: int):
    import torch

    from multidisttorch_amd.models import swd
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(D)
    real, fake = (torch.rand(rows, D, generator=g).to(dev) for _ in range(2))
    dirs = torch.from_numpy(swd.swd_directions(P, D, 0)).to(dev)
    i, j, length = swd.swd_segments(rows, rows, dev)
    seg = (i, j, length.float()[None])
    proj = torch.empty(P, 2 * rows, dtype=torch.float32, device=dev)
    table = torch.empty(P, swd.COLS, dtype=torch.float32, device=dev)
    res = {}
    fns = {
        "swd_project": lambda: C.swd_project(real, fake, dirs, proj),
        "swd_sort": lambda: C.swd_sort(rows, rows, proj, table),
        "swd_rows": lambda: C.swd_rows(real, fake, dirs, proj, table),
        "stock_torch": lambda: res.__setitem__("stock", stock_rows(real, fake, dirs, seg)),
    }
    for f in fns.values():  # warm-up: code objects, GEMM algorithm choice, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev, reps))
    flop = 2.0 * P * 2 * rows * D
    keys = ("swd1", "swd1_se", "swd2", "max_w1")
    ours, stock = swd.swd_stats(table), swd.swd_stats(res["stock"][1])
    out = {"rows": rows, "D": D, "dirs": P, "reps": reps, "kernels": {k: round(ours[k], 6) for k in keys},
           "stock": {k: round(stock[k], 6) for k in keys},
           "max_abs_diff": {"proj": float((proj - res["stock"][0]).abs().max()),
                            "table": float((table - res["stock"][1]).abs().max())},
           "project_flop": flop}
    for k, v in times.items():
        out[k] = _stats(v)
    out["project_tflops"] = round(flop / (out["swd_project"]["median_ms"] * 1e-3) / 1e12, 1)
    out["stock_over_kernels"] = round(out["stock_torch"]["median_ms"] / out["swd_rows"]["median_ms"], 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", default="784,16384")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--dirs", type=int, default=512)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/swd.py measures the HIP backend: no GPU found")
    recs = []
    for D in a.D.split(","):
        r = run(int(D), a.rows, a.dirs, max(5, a.passes), max(1, a.reps))
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
