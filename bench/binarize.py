#!/usr/bin/env python3
"""Time the per-epoch ``--binarize`` refresh (kernel binarize_rows_k).

One process, 60000 rows of 784 and of 16384 pixels (the 28x28 and 128x128
shards), three things alternated round by round after a warm-up of each:

  * ``refresh``: ``_C.binarize_rows`` in ``dynamic`` mode over a shuffled index
    list (a new epoch key every call);
  * ``index_select``: ``torch.index_select(X, 0, idx, out=buf)`` over the same
    rows: a plain gather copy of the same bytes, the yardstick;
  * ``epoch`` (784 only): one epoch of the conv28 step, B = 128, graph-replayed,
    bound to the binarized buffer: what the refresh is added to.

A sample is ``--reps`` back-to-back calls between two device events (the epoch:
one). Prints one JSON line per shape with median / min / max in ms, the bytes
the refresh must move (4 B read + 4 B written per pixel + the index list) over
its median time, and the two ratios refresh / index_select and refresh / epoch.

    python bench/binarize.py [--rows 60000] [--dims 784,16384] [--rounds 7] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "samples": len(v)}


def _event_ms(fn, reps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run(rows: int, D: int, rounds: int, reps: int, B: int = 128):
    import torch

    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(D)
    X = torch.rand(rows, D, device=dev, generator=g)
    idx = torch.randperm(rows, device=dev, generator=g).to(torch.int32)
    idx64 = idx.long()
    buf = torch.empty(rows, D, device=dev)
    epoch = [0]

    def refresh():
        epoch[0] += 1
        C.binarize_rows(X, idx, buf, 1234, epoch[0], 0, "dynamic")

    fns = {"refresh": (refresh, reps), "index_select": (lambda: torch.index_select(X, 0, idx64, out=buf), reps)}
    if D == 784:
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

        tr = ConvVaeTrainer(batch_size=B, image=28, z=32, device=dev, backend="hip", seed=0, use_graphs=True)
        refresh()
        tr.bind_train_data(buf, torch.arange(rows, dtype=torch.int32, device=dev))
        full, tail = rows // B, rows % B
        tr.prepare([B, tail])
        tr.strict_graphs = True

        def one_epoch():
            tr.set_cursor(0, full + (1 if tail else 0))
            tr.train_steps(full, B)
            if tail:
                tr.train_steps(1, tail)

        fns["epoch"] = (one_epoch, 1)
    for f, _ in fns.values():  # warm-up: code objects, allocator, graph upload
        f()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (f, r) in fns.items():
            times[k].append(_event_ms(f, r))
    prop = torch.cuda.get_device_properties(dev)
    out = {"device": prop.name, "arch": getattr(prop, "gcnArchName", ""), "cus": prop.multi_processor_count,
           "rows": rows, "D": D, "reps": reps}
    for k, v in times.items():
        out[k] = _stats(v)
    nbytes = rows * D * 8 + rows * 4
    out["refresh_bytes"] = nbytes
    out["refresh_GBps"] = round(nbytes / (out["refresh"]["median_ms"] * 1e-3) / 1e9, 1)
    out["index_select_GBps"] = round(nbytes / (out["index_select"]["median_ms"] * 1e-3) / 1e9, 1)
    out["refresh_over_index_select"] = round(out["refresh"]["median_ms"] / out["index_select"]["median_ms"], 3)
    if "epoch" in out:
        out["epoch_steps"] = -(-rows // B)
        out["refresh_over_epoch"] = round(out["refresh"]["median_ms"] / out["epoch"]["median_ms"], 5)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--dims", default="784,16384")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/binarize.py measures the HIP kernel: no GPU found")
    recs = []
    for d in a.dims.split(","):
        r = run(a.rows, int(d), max(3, a.rounds), max(1, a.reps))
        recs.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
