#!/usr/bin/env python3
"""Time the latent report pass (``evaluate_latent``).

For the MLP-VAE (Z = 20), the 28x28 conv-VAE (Z = 32) and the 128x128 conv-VAE
(Z = 64): one pass over 10 000 test rows, graph-replayed, after a warm-up pass;
median and spread of ``--passes`` passes. In the same process, alternated with
the pass round by round:

  * ``eager_torch``: the baseline. models/latent.py run eagerly on the GPU in
    fp32 on the pass's own ``mulv`` and eps, chunked over i exactly as the
    trainers' torch backends run it. It does not include the encoder, the pass
    does;
  * ``latent_kernels``: the four once-per-pass launches alone (no encoder);
  * ``latent_pair_k``: the pair kernel alone.

Prints one JSON line per model (times in ms). Nothing here is tuned: the
baseline runs as it ships.

    python bench/latent_eval.py [--models mlp,conv28,conv128] [--rows 10000] [--passes 7] [--out FILE]
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


def run(model: str, rows: int, passes: int):
    import torch

    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models import latent
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
    Z = tr.Z

    res = {}
    res["pass"] = tr.evaluate_latent(X, idx)  # also leaves the buffers the other timings run on
    buf = tr.latent_buffers()
    mu, lv, eps = buf["mulv"][:, :Z].contiguous(), buf["mulv"][:, Z:].contiguous(), buf["eps"]
    chunk = max(1, tr.LATENT_CHUNK_ELEMS // (rows * Z))
    ws, st, hp, prow = tr._lat_workspaces(rows), tr._lat_state(), tr._lat_hparams(), tr._lat_rows

    @torch.no_grad()
    def eager():
        return latent.latent_report(mu, lv, eps, chunk=chunk)

    fns = {
        "evaluate_latent": lambda: res.__setitem__("pass", tr.evaluate_latent(X, idx)),
        "eager_torch": lambda: res.__setitem__("eager", eager()),
        "latent_kernels": lambda: C.latent_report(prow, rows, Z, st, hp, ws),
        "latent_pair_k": lambda: C.latent_pair(prow, rows, Z, st, hp, ws),
    }
    for f in fns.values():  # warm-up: graph capture, code objects, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev))
    p, e = res["pass"], res["eager"]
    out = {"model": model, "batch": B, "rows": rows, "Z": Z, "splits": C.latent_default_splits(rows),
           "eager_chunk_rows": chunk, "graphs": sorted(map(list, tr._lat_graphs)),
           "pass": {k: round(p[k], 4) for k in ("kl", "mi", "tc", "dwkl", "sampled_kl")},
           "eager": {k: round(e[k], 4) for k in ("kl", "mi", "tc", "dwkl", "sampled_kl")},
           "active_units": [p["active_units"], e["active_units"]]}
    for k, v in times.items():
        out[k] = _stats(v)
    m = out["evaluate_latent"]["median_ms"]
    out["eager_over_pass"] = round(out["eager_torch"]["median_ms"] / m, 2)
    out["eager_over_kernels"] = round(out["eager_torch"]["median_ms"] / out["latent_kernels"]["median_ms"], 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mlp,conv28,conv128")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/latent_eval.py measures the HIP backend: no GPU found")
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
