#!/usr/bin/env python3
"""Time the mixture-prior fit (``C.gmm_fit``, csrc/kernels/gmm.hip).

At Z = 20 and Z = 32: ``--rows`` rows drawn from a planted ``--k``-component
mixture (seeded, on the device), ``--iters`` EM iterations from the
deterministic start, after a warm-up round; median and spread of ``--passes``
rounds, each round timing ``--reps`` back-to-back fits between two
synchronisations and reporting the time per fit. In the same process, alternated
round by round:

  * ``gmm_fit``: the whole call, 3 launches per iteration, with its read of the
    status words at the end;
  * ``stock_torch``: the baseline. The same fit from stock float32 torch ops on
    the same device: ``torch.linalg.cholesky``, ``solve_triangular``,
    ``logsumexp``, ``einsum``, batched over the components, with its
    ``[n, K, Z]`` temporaries.

The record also carries the largest difference between the two log-likelihood
histories and both final values. Prints one JSON line per Z (times in ms).
Nothing here is tuned: the baseline runs as it ships.

    python bench/gmm.py [--Z 20,32] [--rows 60000] [--k 10] [--iters 50] [--passes 7] [--reps 5] [--out FILE]
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


def stock_fit(z, K, iters, reg):
    """ll_history [iters + 1] of the fit models/gmm.py defines, from stock torch ops (float32), batched over k."""
    import torch

    n, Z = z.shape
    eye = torch.eye(Z, dtype=z.dtype, device=z.device)
    m = z.mean(0)
    pi = torch.full((K,), 1.0 / K, dtype=z.dtype, device=z.device)
    mu = z[[((2 * k + 1) * n) // (2 * K) for k in range(K)]].clone()
    cov = (z.t() @ z / n - m[:, None] * m[None, :]).expand(K, Z, Z).clone()

    def estep():
        L = torch.linalg.cholesky(cov + reg * eye)
        W = torch.linalg.solve_triangular(L, eye.expand(K, Z, Z), upper=False)
        c = pi.log() - L.diagonal(dim1=1, dim2=2).log().sum(1) - 0.5 * Z * math.log(2.0 * math.pi)
        d = z[:, None, :] - mu[None]
        y = torch.einsum("kij,nkj->nki", W, d)
        lp = c - 0.5 * (y * y).sum(2)
        ll = torch.logsumexp(lp, 1)
        return d, torch.exp(lp - ll[:, None]), ll

    hist = []
    for _ in range(iters):
        d, r, ll = estep()
        hist.append(ll.mean())
        N = r.sum(0)
        rd = r[:, :, None] * d
        dm = rd.sum(0) / N[:, None]
        cov = torch.einsum("nki,nkj->kij", rd, d) / N[:, None, None] - dm[:, :, None] * dm[:, None, :]
        pi, mu = N / n, mu + dm
    hist.append(estep()[2].mean())
    return torch.stack(hist)


def run(Z: int, rows: int, K: int, iters: int, passes: int, reps: int):
    import torch

    from multidisttorch_amd.models import gmm
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(Z)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    centre, A = rnd(K, Z) * (1.5 / math.sqrt(Z)), rnd(K, Z, Z) / math.sqrt(Z)
    comp = torch.arange(rows, device=dev) % K
    z = (centre[comp] + torch.einsum("nij,nj->ni", A[comp], rnd(rows, Z)) + 0.7 * rnd(rows, Z)).contiguous()
    ws = torch.empty(C.gmm_ws_numel(rows, Z, K), dtype=torch.float32, device=dev)
    flat = torch.empty(K * (1 + Z + Z * Z), dtype=torch.float32, device=dev)
    hist = torch.empty(iters + 1, dtype=torch.float32, device=dev)
    res = {}
    fns = {
        "gmm_fit": lambda: C.gmm_fit(z, K, iters, ws, flat, hist),
        "stock_torch": lambda: res.__setitem__("stock", stock_fit(z, K, iters, gmm.REG_COVAR)),
    }
    for f in fns.values():  # warm-up: code objects, solver handles, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev, reps))
    out = {"rows": rows, "Z": Z, "K": K, "iters": iters, "reps": reps,
           "ll_final": {"kernels": round(float(hist[-1]), 6), "stock": round(float(res["stock"][-1]), 6)},
           "max_abs_diff_ll_history": float((hist - res["stock"]).abs().max()),
           "launches_per_fit": 3 * iters + 4}
    for k, v in times.items():
        out[k] = _stats(v)
    out["gmm_fit_ms_per_iter"] = round(out["gmm_fit"]["median_ms"] / max(iters, 1), 4)
    out["stock_over_kernels"] = round(out["stock_torch"]["median_ms"] / out["gmm_fit"]["median_ms"], 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--Z", default="20,32")
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/gmm.py measures the HIP backend: no GPU found")
    recs = []
    for Z in a.Z.split(","):
        r = run(int(Z), a.rows, a.k, a.iters, max(5, a.passes), max(1, a.reps))
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
