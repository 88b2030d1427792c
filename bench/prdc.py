#!/usr/bin/env python3
"""Time the PRDC pass (``evaluate_samples(prdc_k=5)``).

For the MLP-VAE (D = 784) and the 128x128 conv-VAE (D = 16384): n decoded prior
samples against n rows, k = 5, after a warm-up round; median and spread of
``--passes`` rounds. In the same process, alternated round by round:

  * ``prdc_rows``: the five launches of csrc/kernels/prdc.hip alone, on the
    pass's own real and generated rows;
  * ``two_sample_rows``: the sample report's kernels on the same rows (the pair
    counts put PRDC near 1.5 times their work);
  * ``evaluate_samples``: the whole pass with ``prdc_k=5`` (sample report and
    PRDC: gather, host z, decoder, both kernel families, final reductions);
  * ``stock_torch``: the baseline. The same per-row table from stock torch ops on
    the same device in float32: row norms, the Gram product by ``torch.mm`` in
    row chunks, ``kthvalue``, compare and sum. It does not include the decoder.

The record also carries the largest difference between the two tables and the
four statistics from each. Prints one JSON line per model (times in ms). Nothing
here is tuned: the baseline runs as it ships.

    python bench/prdc.py [--models mlp,conv128] [--rows 10000] [--passes 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {"mlp": dict(image=28, batch=128), "conv28": dict(image=28, batch=128), "conv128": dict(image=128, batch=32)}
STOCK_CHUNK = 2048  # rows per torch.mm: a [2048, n] float32 block and its temporaries
K = 5


def _timed(fn, dev):
    import torch

    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def _stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "passes": len(v)}


def stock_rows(real, fake, k, chunk=STOCK_CHUNK):
    """The per-row table from stock torch ops (float32, Gram by torch.mm)."""
    import torch

    def d2_blocks(A, B):
        qa, qb = (A * A).sum(1), (B * B).sum(1)
        for i0 in range(0, A.shape[0], chunk):
            yield i0, (qa[i0: i0 + chunk, None] + qb[None] - 2.0 * torch.mm(A[i0: i0 + chunk], B.t())).clamp_min_(0.0)

    def radii(X):
        cols = torch.arange(X.shape[0], device=X.device)
        return torch.cat([d2.masked_fill_(cols[None] == cols[i0: i0 + d2.shape[0], None], float("inf"))
                         .kthvalue(k, dim=1).values for i0, d2 in d2_blocks(X, X)])

    rr, rf = radii(real), radii(fake)
    cnt_f = torch.zeros_like(rf)
    dmin_f = torch.full_like(rf, float("inf"))
    cnt_r, dmin_r = [], []
    for i0, d2 in d2_blocks(real, fake):
        cnt_r.append((d2 <= rf[None]).sum(1).float())
        dmin_r.append(d2.min(1).values)
        cnt_f += (d2 <= rr[i0: i0 + d2.shape[0], None]).sum(0).float()
        dmin_f = torch.minimum(dmin_f, d2.min(0).values)
    return torch.stack([torch.cat([rr, rf]), torch.cat(cnt_r + [cnt_f]), torch.cat(dmin_r + [dmin_f])], 1)


def run(model: str, rows: int, passes: int):
    import torch

    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models import prdc
    from multidisttorch_amd.models import sample_report as sr
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    image, B = MODELS[model]["image"], MODELS[model]["batch"]
    Xtr = synthetic_images(4 * B, size=image, seed=1, device=dev)
    X = synthetic_images(rows, size=image, seed=2, device=dev)
    idx = torch.arange(rows, dtype=torch.int32, device=dev)
    if model == "mlp":
        from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

        tr = MlpVaeTrainer(batch_size=B, device=dev, backend="hip", seed=0, use_graphs=True)
    else:
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

        tr = ConvVaeTrainer(batch_size=B, image=image, z=32 if image == 28 else 64, device=dev, backend="hip", seed=0,
                            use_graphs=True)
    tr.bind_train_data(Xtr, torch.arange(4 * B, dtype=torch.int32, device=dev))
    tr.set_cursor(0, 4)
    tr.train_steps(20)

    res = {}
    first = tr.evaluate_samples(X, idx, return_rows=True, prdc_k=K)  # also leaves the rows the other timings run on
    real, fake, h = first["real"], first["fake"], first["bandwidths"]
    D = real.shape[1]
    ws = torch.empty(C.prdc_ws_numel(rows, rows, D, K), dtype=torch.float32, device=dev)
    table = torch.empty(2 * rows, prdc.COLS, dtype=torch.float32, device=dev)
    ts_ws = torch.empty(C.two_sample_ws_numel(rows, rows, D), dtype=torch.float32, device=dev)
    ts_table = torch.empty(2 * rows, sr.COLS, dtype=torch.float32, device=dev)

    fns = {
        "prdc_rows": lambda: C.prdc_rows(real, fake, K, ws, table),
        "two_sample_rows": lambda: C.two_sample_rows(real, fake, h, ts_ws, ts_table),
        "evaluate_samples": lambda: res.__setitem__("pass", tr.evaluate_samples(X, idx, prdc_k=K)),
        "stock_torch": lambda: res.__setitem__("stock", stock_rows(real, fake, K)),
    }
    for f in fns.values():  # warm-up: code objects, GEMM algorithm choice, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev))
    diff = (table - res["stock"]).abs()
    gram_flop = 2.0 * 3 * rows ** 2 * D  # real x real, fake x fake, real x fake
    keys = ("precision", "recall", "density", "coverage")
    stock = prdc.prdc_stats(res["stock"], rows, rows, K)
    out = {"model": model, "rows": rows, "D": D, "k": K, "strips": C.prdc_strips(rows, rows), "stock_chunk_rows": STOCK_CHUNK,
           "pass": {k: round(res["pass"]["prdc"][k], 6) for k in keys}, "stock": {k: round(stock[k], 6) for k in keys},
           "table_max_abs_diff": {"rad": float(diff[:, 0].max()), "cnt": float(diff[:, 1].max()),
                                  "dminx": float(diff[:, 2].max())},
           "gram_flop": gram_flop}
    for k, v in times.items():
        out[k] = _stats(v)
    out["kernels_gram_tflops"] = round(gram_flop / (out["prdc_rows"]["median_ms"] * 1e-3) / 1e12, 1)
    out["stock_over_kernels"] = round(out["stock_torch"]["median_ms"] / out["prdc_rows"]["median_ms"], 2)
    out["prdc_over_two_sample"] = round(out["prdc_rows"]["median_ms"] / out["two_sample_rows"]["median_ms"], 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mlp,conv128")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/prdc.py measures the HIP backend: no GPU found")
    recs = []
    for m in a.models.split(","):
        r = run(m.strip(), a.rows, max(5, a.passes))
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
