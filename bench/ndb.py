#!/usr/bin/env python3
"""Time the k-means kernels behind ``--ndb`` (``C.kmeans_rows``, csrc/kernels/kmeans.hip).

At D = 784 and D = 16384: ``--rows`` real against ``--rows`` generated rows
(uniform random pixels: every launch does the same work whatever the values,
the iteration count is fixed), K bins, T iterations from ``ndb_init_idx``, after
a warm-up round; median and spread of ``--passes`` rounds, each round timing
``--reps`` back-to-back calls between two synchronisations and reporting the
time per call. In the same process, alternated round by round:

  * ``kmeans_assign`` and ``kmeans_update``: one step alone on the real rows (the
    first with its two small fold launches, the second with its fold);
  * ``kmeans_rows``: the whole fit, 3 T + 3 launches;
  * ``stock_torch``: the baseline. The same fit from stock float32 torch ops on
    the same device: ``torch.mm``, ``argmin``, ``index_add_``, ``bincount``, with
    no host synchronisation inside the loop either.

The record also carries the share of rows on which the two fits' labels agree
(uniform rows have near ties, which float32 Gram forms in two orders may break
differently), the statistics from each and the bytes and operations one
iteration needs. Prints one JSON line per D (times in ms). Nothing here is tuned:
the baseline runs as it ships.

    python bench/ndb.py [--D 784,16384] [--rows 10000] [--K 100] [--iters 20] [--passes 7] [--reps 5] [--out FILE]
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


def stock_fit(real, fake, K, T, init):
    """(labels, mind, centroids, moved, inertia) from stock torch ops (float32)."""
    import torch

    def assign(x, c):
        v, lab = ((c * c).sum(1)[None] - 2.0 * torch.mm(x, c.t())).min(1)
        return lab, v

    cent = real[init].clone()
    label = torch.full((real.shape[0],), -1, dtype=torch.int64, device=real.device)
    moved = []
    for _ in range(T):
        new, _ = assign(real, cent)
        moved.append((new != label).sum())
        label = new
        cnt = torch.bincount(label, minlength=K)
        s = torch.zeros_like(cent).index_add_(0, label, real)
        cent = torch.where((cnt > 0)[:, None], s / cnt.clamp(min=1)[:, None], cent)
    x = torch.cat([real, fake])
    labels, v = assign(x, cent)
    mind = ((x * x).sum(1) + v).clamp(min=0)
    return labels, mind, cent, torch.stack(moved), mind[: real.shape[0]].double().sum()


def run(D: int, rows: int, K: int, T: int, passes: int, reps: int):
    import torch

    from multidisttorch_amd.models import ndb
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(D)
    real, fake = (torch.rand(rows, D, generator=g).to(dev) for _ in range(2))
    init = ndb.ndb_init_idx(rows, K, 0).to(dev)
    ws = torch.empty(C.kmeans_ws_numel(rows, rows, D, K), dtype=torch.float32, device=dev)
    cent0 = real[init].contiguous()
    lab0 = C.kmeans_assign(real, None, cent0, ws)[0]
    res = {}
    fns = {
        "kmeans_assign": lambda: C.kmeans_assign(real, None, cent0, ws),
        "kmeans_update": lambda: C.kmeans_update(real, lab0, cent0, ws),
        "kmeans_rows": lambda: res.__setitem__("ours", C.kmeans_rows(real, fake, K, T, init, ws)),
        "stock_torch": lambda: res.__setitem__("stock", stock_fit(real, fake, K, T, init)),
    }
    for f in fns.values():  # warm-up: code objects, GEMM algorithm choice, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev, reps))
    ours, stock = res["ours"], res["stock"]
    keys = ("ndb", "jsd", "missing", "inertia", "moved")
    st = lambda r: {k: v for k, v in ndb.ndb_stats(r[0], rows, K, float(r[4]), int(r[3][-1]), T).items() if k in keys}
    out = {"rows": rows, "D": D, "K": K, "iters": T, "reps": reps, "kernels": st(ours), "stock": st(stock),
           "labels_agree": round(float((ours[0].long() == stock[0]).float().mean()), 6),
           "band": C.kmeans_layout(rows)["band"], "final_band": C.kmeans_layout(2 * rows)["band"],
           # one iteration: X read by the assign and by the update; the Gram product and the one-hot product
           "iter_bytes": 2.0 * 4 * rows * D, "assign_flop": 2.0 * rows * K * D}
    for k, v in times.items():
        out[k] = _stats(v)
    out["assign_tflops"] = round(out["assign_flop"] / (out["kmeans_assign"]["median_ms"] * 1e-3) / 1e12, 2)
    out["update_gbps"] = round(4.0 * rows * D / (out["kmeans_update"]["median_ms"] * 1e-3) / 1e9, 1)
    out["stock_over_kernels"] = round(out["stock_torch"]["median_ms"] / out["kmeans_rows"]["median_ms"], 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", default="784,16384")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/ndb.py measures the HIP backend: no GPU found")
    recs = []
    for D in a.D.split(","):
        r = run(int(D), a.rows, a.K, a.iters, max(5, a.passes), max(1, a.reps))
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
