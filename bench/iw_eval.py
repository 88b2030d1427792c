#!/usr/bin/env python3
"""Time the importance-weighted test log-likelihood pass (``evaluate_iw``).

For the MLP-VAE (B = 128) and the 28x28 conv-VAE: K = 50 samples over 10 000
test rows, graph-replayed, after a warm-up pass; median and spread of
``--passes`` passes. Two baselines in the same process, alternated with the
pass round by round:

  * ``k_evaluate``: K consecutive ``evaluate()`` passes, all a user could do
    without ``evaluate_iw`` (K encoder runs, one draw each, and still no
    per-row combination of the draws);
  * ``eager_torch``: models/iw.py run eagerly on the GPU in fp32 on the same
    weights (noise from ``torch.randn``: the host Philox generator would time
    the CPU; the arithmetic per draw is the same).

Prints one JSON line per model (times in ms). Nothing here is tuned: the
baselines run as they ship.

    python bench/iw_eval.py [--models mlp,conv28] [--k 50] [--rows 10000] [--passes 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def run(model: str, K: int, rows: int, passes: int, B: int):
    import torch

    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models import iw

    dev = torch.device("cuda", 0)
    Xtr = synthetic_images(4 * B, seed=1, device=dev)
    X = synthetic_images(rows, seed=2, device=dev)
    idx = torch.arange(rows, dtype=torch.int32, device=dev)
    if model == "mlp":
        from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

        tr = MlpVaeTrainer(batch_size=B, device=dev, backend="hip", seed=0, use_graphs=True)
    else:
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer, TorchConvVAE

        tr = ConvVaeTrainer(batch_size=B, image=28, z=32, device=dev, backend="hip", seed=0, use_graphs=True)
    tr.bind_train_data(Xtr, torch.arange(4 * B, dtype=torch.int32, device=dev))
    tr.set_cursor(0, 4)
    tr.train_steps(20)

    # the eager baseline's model: the same weights in stock torch ops, fp32
    if model == "mlp":
        v = {k: t.clone() for k, t in tr.named_parameters().items()}
        logw = lambda x, eps: iw.mlp_iw_log_weights(v, x, eps)[0]
    else:
        ref = TorchConvVAE(tr.spec, tr.image, tr.channels, tr.Z).to(dev)
        ref.from_arena(tr.named_parameters())

        def logw(x, eps):
            mu, lv = ref.encode(x)
            dec = lambda z: ref.decode_logits(z).permute(0, 2, 3, 1).reshape(z.shape[0], tr.D)
            return iw.iw_log_weights(mu, lv, eps, x, dec)[0]

    # samples per eager decoder call: the pass's own chunking (conv: one full batch of rows per decoder run)
    S = iw.default_chunk(K, B) if model == "mlp" else 1

    @torch.no_grad()
    def eager():
        tot = torch.zeros(2, dtype=torch.float64, device=dev)
        for b in range(0, rows, B):
            x = X[b: b + B]
            eps = torch.randn(K, x.shape[0], tr.Z, device=dev)
            lw = torch.cat([logw(x, eps[s: s + S]) for s in range(0, K, S)], 0)
            a, e = iw.iw_reduce(lw)
            tot[0] += a.double().sum()
            tot[1] += e.double().sum()
        return tot.tolist()

    res = {}
    fns = {
        "evaluate_iw": lambda: res.__setitem__("iw", tr.evaluate_iw(X, idx, K)),
        "k_evaluate": lambda: [tr.evaluate(X, idx, want_first_recon=False) for _ in range(K)],
        "one_evaluate": lambda: tr.evaluate(X, idx, want_first_recon=False),
        "eager_torch": lambda: res.__setitem__("eager", eager()),
    }
    for f in fns.values():  # warm-up: graph capture, code objects, allocator
        f()
    times = {k: [] for k in fns}
    for _ in range(passes):
        for k, f in fns.items():
            times[k].append(_timed(f, dev))
    out = {"model": model, "batch": B, "k": K, "rows": rows, "chunk_samples": S,
           "iw_nll": round(res["iw"]["nll"] / rows, 4), "iw_neg_elbo": round(res["iw"]["neg_elbo"] / rows, 4),
           "eager_nll": round(res["eager"][0] / rows, 4)}
    for k, v in times.items():
        out[k] = _stats(v)
    m = out["evaluate_iw"]["median_ms"]
    out["k_evaluate_over_iw"] = round(out["k_evaluate"]["median_ms"] / m, 2)
    out["eager_over_iw"] = round(out["eager_torch"]["median_ms"] / m, 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mlp,conv28")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/iw_eval.py measures the HIP backend: no GPU found")
    recs = []
    for m in a.models.split(","):
        r = run(m.strip(), a.k, a.rows, max(5, a.passes), a.batch_size)
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
