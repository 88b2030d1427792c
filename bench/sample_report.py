#!/usr/bin/env python3
"""Time the sample report pass (``evaluate_samples``).

For the MLP-VAE (D = 784) and the 128x128 conv-VAE (D = 16384): n decoded prior
samples against n rows, after a warm-up round; median and spread of ``--passes``
rounds. In the same process, alternated round by round:

  * ``two_sample_rows``: the three launches of csrc/kernels/two_sample.hip alone,
    on the pass's own real and generated rows;
  * ``evaluate_samples``: the whole pass (gather, bandwidths, host z, decoder,
    kernels, final reductions);
  * ``stock_torch``: the baseline. The same per-row table from stock torch ops on
    the same device in float32: row norms, the Gram product by ``torch.mm`` in
    row chunks, then clamp / mask / min / exp / sum per chunk. It does not
    include the decoder either.

The record also carries the largest difference between the two tables, the
operations the Gram product needs and the kernels' rate over them. Prints one
JSON line per model (times in ms). Nothing here is tuned: the baseline runs as
it ships.

    python bench/sample_report.py [--models mlp,conv128] [--rows 10000] [--passes 7] [--out FILE]
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
STOCK_CHUNK = 2048  # rows of the union per torch.mm: a [2048, 2n] float32 block and its temporaries


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


def stock_rows(real, fake, h, chunk=STOCK_CHUNK):
    """The per-row table from stock torch ops (float32, Gram by torch.mm)."""
    import torch

    na = real.shape[0]
    U = torch.cat([real, fake])
    N = U.shape[0]
    q = (U * U).sum(1)
    cols = torch.arange(N, device=U.device)
    out = []
    for i0 in range(0, N, chunk):
        Ui = U[i0: i0 + chunk]
        d2 = (q[i0: i0 + chunk, None] + q[None] - 2.0 * torch.mm(Ui, U.t())).clamp_min_(0.0)
        self_ = cols[None] == cols[i0: i0 + chunk, None]
        dm = d2.masked_fill(self_, float("inf"))
        row = [dm[:, :na].min(1).values, dm[:, na:].min(1).values]
        ks = [torch.exp(d2 * (-1.0 / hs)).masked_fill_(self_, 0.0) for hs in h]
        row += [k[:, :na].sum(1) for k in ks] + [k[:, na:].sum(1) for k in ks]
        out.append(torch.stack(row, 1))
    return torch.cat(out)


def run(model: str, rows: int, passes: int):
    import torch

    from multidisttorch_amd.data.datasets import synthetic_images
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
    first = tr.evaluate_samples(X, idx, return_rows=True)  # also leaves the rows the other timings run on
    real, fake, h = first["real"], first["fake"], first["bandwidths"]
    D = real.shape[1]
    ws = torch.empty(C.two_sample_ws_numel(rows, rows, D), dtype=torch.float32, device=dev)
    table = torch.empty(2 * rows, sr.COLS, dtype=torch.float32, device=dev)

    fns = {
        "two_sample_rows": lambda: C.two_sample_rows(real, fake, h, ws, table),
        "evaluate_samples": lambda: res.__setitem__("pass", tr.evaluate_samples(X, idx)),
        "stock_torch": lambda: res.__setitem__("stock", stock_rows(real, fake, h)),
    }
    for f in fns.values():  # warm-up: code objects, GEMM algorithm choice, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev))
    p = res["pass"]
    stock = sr.sample_stats(res["stock"], rows, rows)
    diff = (table - res["stock"]).abs()
    gram_flop = 2.0 * (2 * rows) ** 2 * D
    out = {"model": model, "rows": rows, "D": D, "strips": C.two_sample_strips(rows, rows), "stock_chunk_rows": STOCK_CHUNK,
           "pass": {k: round(p[k], 6) for k in ("mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake", "rf_asym")},
           "stock": {k: round(stock[k], 6) for k in ("mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake", "rf_asym")},
           "table_max_abs_diff": {"dmin": float(diff[:, :2].max()), "ksum": float(diff[:, 2:].max())},
           "gram_flop": gram_flop}
    for k, v in times.items():
        out[k] = _stats(v)
    out["kernels_gram_tflops"] = round(gram_flop / (out["two_sample_rows"]["median_ms"] * 1e-3) / 1e12, 1)
    out["stock_over_kernels"] = round(out["stock_torch"]["median_ms"] / out["two_sample_rows"]["median_ms"], 2)
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
        raise SystemExit("bench/sample_report.py measures the HIP backend: no GPU found")
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
