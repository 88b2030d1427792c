#!/usr/bin/env python3
"""Time the reconstruction report pass (``evaluate_recon``).

For the MLP-VAE (28x28) and the 128x128 conv-VAE: n test rows against their
reconstructions from the posterior mean, after a warm-up round; median and
spread of ``--passes`` rounds. In the same process, alternated round by round:

  * ``recon_rows``: the launches of csrc/kernels/recon.hip alone on the pass's
    own rows, ``--reps`` calls back to back per timing (one call at 28x28 is
    shorter than a launch), reported per call;
  * ``evaluate_recon``: the whole pass (gather, encoder, decoder, kernels, final
    reductions);
  * ``stock_torch``: the baseline. The same table from stock float32 torch ops on
    the same device: ``F.conv2d`` with the 11x11 window over the five stacked
    maps, in row chunks (models/recon_report.py, as the torch backend runs it).
    It includes neither encoder nor decoder, and runs once per timing.

The record also carries the largest difference between the two tables per column
and the kernels' achieved bytes per second against the compulsory traffic: both
images read once, ``2 n S^2 * 4`` bytes. Prints one JSON line per model (times in
ms). Nothing here is tuned: the baseline runs as it ships.

    python bench/recon_report.py [--models mlp,conv128] [--rows 10000] [--passes 7] [--reps 20] [--out FILE]
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


def _timed(fn, dev, reps=1):
    import torch

    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3 / reps


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "passes": len(v)}


def run(model: str, rows: int, passes: int, reps: int):
    import torch

    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models import recon_report as rr
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
    first = tr.evaluate_recon(X, idx, return_rows=True)  # also leaves the rows the other timings run on
    real, recon = first["real"], first["recon"]
    ws = torch.empty(C.recon_ws_numel(rows, image), dtype=torch.float32, device=dev)
    table = torch.empty(rows, rr.COLS, dtype=torch.float32, device=dev)
    fns = {
        "recon_rows": (lambda: C.recon_rows(real, recon, image, ws, table), reps),
        "evaluate_recon": (lambda: res.__setitem__("pass", tr.evaluate_recon(X, idx)), 1),
        "stock_torch": (lambda: res.__setitem__("stock", rr.recon_rows(real, recon, image)), 1),
    }
    for f, _ in fns.values():  # warm-up: code objects, convolution algorithm choice, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, (f, r) in fns.items():
            times[k].append(_timed(f, dev, r))
    diff = (table - res["stock"]).abs().amax(0).tolist()
    keys = ("mse", "psnr", "ssim", "ssim_l", "ssim_cs", "ssim_min")
    stock = rr.recon_stats(res["stock"], image)
    nbytes = 2.0 * rows * image * image * 4
    out = {"model": model, "rows": rows, "side": image, "bands": C.recon_bands(image), "reps": reps,
           "pass": {k: round(res["pass"][k], 6) for k in keys}, "stock": {k: round(stock[k], 6) for k in keys},
           "table_max_abs_diff": dict(zip(("se", "ssim", "l", "cs"), diff)), "compulsory_bytes": nbytes}
    for k, v in times.items():
        out[k] = _stats(v)
    out["kernels_gb_per_s"] = round(nbytes / (out["recon_rows"]["median_ms"] * 1e-3) / 1e9, 1)
    out["stock_over_kernels"] = round(out["stock_torch"]["median_ms"] / out["recon_rows"]["median_ms"], 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mlp,conv128")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/recon_report.py measures the HIP backend: no GPU found")
    recs = []
    for m in a.models.split(","):
        r = run(m.strip(), a.rows, max(5, a.passes), max(1, a.reps))
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
