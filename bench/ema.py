#!/usr/bin/env python3
"""Time weight averaging (``ema_decay``): the step with and without the average,
the ``ema_update`` launch alone, and an ``averaged_weights()`` enter plus exit.

For the MLP-VAE (B = 128, Z = 20), the 28x28 conv-VAE (B = 128, Z = 32, the
fused step) and the 128x128 conv-VAE (B = 64, Z = 64): ``--steps`` graph-replayed
steps per round after a warm-up, the trainer without and with the average
alternated round by round in one process; median and spread over ``--rounds``
rounds, in microseconds per step.

In the same process, round by round as well, over the model's own arena size n:

  * ``ema_update``: the launch alone, back to back (12 bytes per element);
  * ``swap_12B``: ``arena_swap`` over 3n/4 elements: the same launch shape
    (float4 lanes, 256 threads, the same grid rule) moving the same 12n bytes
    as plain loads and stores, nothing computed;
  * ``torch_copy_12B``: ``dst.copy_(src)`` over 3n/2 floats (6n bytes read, 6n written);
  * ``averaged_enter_exit``: ``with trainer.averaged_weights(): pass`` (two
    swaps and two refreshes of the derived weight copies);
  * ``test_pass``: one ``evaluate`` over 10 000 rows, for scale.

Prints one JSON line per model. For the kernel's own time take a kernel trace
in a run of its own:

    rocprofv3 --kernel-trace --stats -- python bench/ema.py --models mlp --rounds 2

    python bench/ema.py [--models mlp,conv28,conv128] [--steps 200] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {"mlp": dict(image=28, batch=128), "conv28": dict(image=28, batch=128), "conv128": dict(image=128, batch=64)}
DECAY = 0.999
TEST_ROWS = 10000


def _timed(fn, dev, n):
    import torch

    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e6 / n


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def _trainer(model, dev, **kw):
    B, image = MODELS[model]["batch"], MODELS[model]["image"]
    if model == "mlp":
        from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

        return MlpVaeTrainer(batch_size=B, device=dev, backend="hip", seed=0, use_graphs=True, graph_steps=20, **kw)
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    return ConvVaeTrainer(batch_size=B, image=image, z=64 if image == 128 else 32, device=dev, backend="hip", seed=0,
                          use_graphs=True, graph_steps=20, **kw)


def run(model: str, steps: int, rounds: int):
    import torch

    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    B, image = MODELS[model]["batch"], MODELS[model]["image"]
    X = synthetic_images(8 * B, size=image, seed=1, device=dev)
    idx = torch.arange(8 * B, device=dev, dtype=torch.int32)
    trainers = {"plain": _trainer(model, dev), "ema": _trainer(model, dev, ema_decay=DECAY)}
    for tr in trainers.values():
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, 8)
        tr.prepare([B])
        tr.train_steps(steps)  # warm-up
    te = trainers["ema"]
    n = te.numel
    n_test = TEST_ROWS if image == 28 else 2000   # 128x128 rows are 64 KiB each
    Xt = synthetic_images(n_test, size=image, seed=2, device=dev)
    it = torch.arange(n_test, device=dev, dtype=torch.int32)
    e, p = torch.randn(n, device=dev), torch.randn(n, device=dev)
    m = (3 * n // 4) // 4 * 4
    sa, sb = torch.randn(m, device=dev), torch.randn(m, device=dev)
    ca, cb = torch.randn(3 * n // 2, device=dev), torch.randn(3 * n // 2, device=dev)
    reps = 200

    def kernel():
        for _ in range(reps):
            C.ema_update(e, p, n, decay=DECAY, t=1000)

    def swap():
        for _ in range(reps):
            C.arena_swap(sa, sb, m)

    def copy():
        for _ in range(reps):
            cb.copy_(ca)

    def enter_exit():
        for _ in range(10):
            with te.averaged_weights():
                pass

    def test_pass():
        te.evaluate(Xt, it, want_first_recon=False)

    for f in (kernel, swap, copy, enter_exit, test_pass):
        f()
    times = {k: [] for k in list(trainers) + ["ema_update", "swap_12B", "torch_copy_12B", "averaged_enter_exit",
                                              "test_pass"]}
    for _ in range(rounds):
        for k, tr in trainers.items():
            times[k].append(_timed(lambda tr=tr: tr.train_steps(steps), dev, steps))
        times["ema_update"].append(_timed(kernel, dev, reps))
        times["swap_12B"].append(_timed(swap, dev, reps))
        times["torch_copy_12B"].append(_timed(copy, dev, reps))
        times["averaged_enter_exit"].append(_timed(enter_exit, dev, 10))
        times["test_pass"].append(_timed(test_pass, dev, 1))
    out = {"model": model, "B": B, "arena_floats": n, "steps": steps, "rounds": rounds, "decay": DECAY,
           "test_rows": n_test}
    out.update({k: _stats(v) for k, v in times.items()})
    out["step_cost_us"] = round(out["ema"]["median_us"] - out["plain"]["median_us"], 2)
    out["kernel_over_swap"] = round(out["ema_update"]["median_us"] / out["swap_12B"]["median_us"], 3)
    out["kernel_GBps"] = round(12.0 * n / out["ema_update"]["median_us"] / 1e3, 1)
    out["same_params"] = bool(torch.equal(trainers["plain"].params, te.params))  # the average leaves training alone
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mlp,conv28,conv128")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for m in a.models.split(","):
        r = run(m.strip(), a.steps, a.rounds)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
