#!/usr/bin/env python3
"""Time the training step with and without the total-correlation penalty.

For the MLP-VAE (B = 128, Z = 20), the 28x28 conv-VAE (B = 128, Z = 32: the
layer path for both weights, plus the fused step at weight 0 for reference) and
the 128x128 conv-VAE (B = 64, Z = 64): ``--steps`` graph-replayed steps per
round after a warm-up, ``tc_weight`` 0 and 3 alternated round by round in one
process; median and spread over ``--rounds`` rounds, in microseconds per step.

In the same process, round by round as well:

  * ``tc_kernels``: the penalty's launches alone (pack, pair, merge, backward,
    fold) on the step's own mulv and eps, back to back;
  * ``eager_torch``: the baseline. The same value and gradient by autograd
    through models/latent.py, run eagerly on the GPU in fp32 on the same rows.

Prints one JSON line per model. Nothing here is tuned: the baseline runs as it
ships. For the launches one by one, take a kernel trace in a run of its own:

    rocprofv3 --kernel-trace --stats -- python bench/tc_penalty.py --models mlp --rounds 2

    python bench/tc_penalty.py [--models mlp,conv28,conv128] [--steps 200] [--rounds 5] [--out FILE]
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
WEIGHT = 3.0


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
    from multidisttorch_amd.models import tc
    from multidisttorch_amd.ops import native

    C = native.require()
    dev = torch.device("cuda", 0)
    B, image = MODELS[model]["batch"], MODELS[model]["image"]
    X = synthetic_images(8 * B, size=image, seed=1, device=dev)
    idx = torch.arange(8 * B, device=dev, dtype=torch.int32)
    forms = {"tc0": {}, "tc3": dict(tc_weight=WEIGHT)}
    if model == "conv28":
        # weight 0 on the layer path too (the penalty's own path), the fused step for reference
        os.environ["MDT_CONV_F28"] = "0"
    trainers = {k: _trainer(model, dev, **kw) for k, kw in forms.items()}
    if model == "conv28":
        del os.environ["MDT_CONV_F28"]
        trainers["tc0_fused"] = _trainer(model, dev)
        assert trainers["tc0_fused"].f28 and not trainers["tc0"].f28 and not trainers["tc3"].f28
    for tr in trainers.values():
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, 8)
        tr.prepare([B])
        tr.train_steps(steps)  # warm-up
    t3 = trainers["tc3"]
    Z = t3.Z
    mulv = (t3.engine.act("mulv", B) if model == "mlp" else t3.mulv[:B]).clone()
    eps = (t3.engine.act("eps", B) if model == "mlp" else t3.eps[:B]).clone()
    ws = torch.zeros(C.tc_ws_numel(B, Z), device=dev)
    value = torch.zeros(1, dtype=torch.float64, device=dev)
    add = torch.zeros(B, 2 * Z, device=dev)
    w = torch.tensor([WEIGHT], device=dev)
    reps = 50

    def kernels():
        for _ in range(reps):
            C.tc_penalty(mulv, eps, B, Z, ws, value, weight=w, add_out=add)

    def eager():
        mu, lv = mulv[:, :Z].clone().requires_grad_(), mulv[:, Z:].clone().requires_grad_()
        (WEIGHT * tc.tc_batch(mu, lv, eps)).backward()

    kernels()
    eager()
    times = {k: [] for k in list(trainers) + ["tc_kernels", "eager_torch"]}
    for _ in range(rounds):
        for k, tr in trainers.items():
            times[k].append(_timed(lambda tr=tr: tr.train_steps(steps), dev, steps))
        times["tc_kernels"].append(_timed(kernels, dev, reps))
        times["eager_torch"].append(_timed(eager, dev, 1))
    out = {"model": model, "B": B, "Z": Z, "steps": steps, "rounds": rounds, "splits": C.tc_default_splits(B, Z)}
    out.update({k: _stats(v) for k, v in times.items()})
    out["step_cost_us"] = round(out["tc3"]["median_us"] - out["tc0"]["median_us"], 2)
    out["train_tc_per_row"] = t3.read_state()["epoch_tc"] / max(1, t3.read_state()["step"] * B)
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
