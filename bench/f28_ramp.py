#!/usr/bin/env python3
"""Dispatch ramp of the fused 28x28 step's launch (one MI355X).

Part 1, the step itself: the paired step's entry stamps (slot 0 of every
workgroup, s_memrealtime at 100 MHz) against block id, role and XCD
(block id % 8: round-robin dispatch, checked against the probe's XCC ids in
part 2): the start-time map of the launch whose first-entry-to-last-entry
skew the phase tool reports.

Part 2, an empty kernel of the same launch shape (``_C.probe_ramp``,
csrc/kernels/probe.hip), one resource changed at a time: static LDS bytes
per workgroup (the step's / 64 KB / 0) and threads per workgroup
(512 / 256). It does no work: it only tells which resource sets the ramp.

    python bench/f28_ramp.py [--batch 128] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP_LDS = 161216


def step_map(B, steps):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    dev = torch.device("cuda", 0)
    tr = ConvVaeTrainer(batch_size=B, image=28, device=dev, backend="hip", seed=0, use_graphs=False)
    assert tr.f28 and tr.f28_merge and tr.f28_pair
    st = torch.zeros(2 * B * 16, dtype=torch.int64, device=dev)
    tr.f28_stamps = (st, None)
    X = synthetic_images(8 * B, device=dev)
    tr.bind_train_data(X, torch.arange(8 * B, device=dev, dtype=torch.int32))
    tr.set_cursor(0, 8)
    out = []
    for _ in range(steps):
        st.zero_()
        tr.train_steps(1)
        torch.cuda.synchronize()
        s = st.view(2 * B, 16).cpu().numpy()
        start = (s[:, 0] - s[:, 0].min()) * 0.01
        out.append({"start_us": start.tolist(), "mode": (s[:, 15] & 15).tolist()})
    return out


def print_step_map(m, B):
    start, mode = np.array(m["start_us"]), np.array(m["mode"])
    blk = np.arange(2 * B)
    print(f"step launch, {2 * B} workgroups: first entry -> last entry {start.max():.2f} us")
    print("  by block-id group of 32 (min / median / max start, us):")
    for g in range(0, 2 * B, 32):
        v = start[g:g + 32]
        print(f"    blocks {g:3d}-{g + 31:3d}: {v.min():5.2f} {np.median(v):5.2f} {v.max():5.2f}")
    print("  by XCD (block id % 8):")
    for x in range(8):
        v = start[blk % 8 == x]
        print(f"    XCD {x}: {v.min():5.2f} {np.median(v):5.2f} {v.max():5.2f}")
    print("  by role (slot 15: 1 = role 0, 2 = role 1):")
    for r in (1, 2):
        v = start[mode == r]
        if len(v):
            print(f"    mode {r}: n={len(v)} {v.min():5.2f} {np.median(v):5.2f} {v.max():5.2f}")
    order = np.argsort(start)
    print("  first 8 blocks to start:", order[:8].tolist(), " last 8:", order[-8:].tolist())


def probe(C, blocks, threads, lds, reps):
    out = torch.zeros(blocks, 2, dtype=torch.int64, device="cuda")
    skews, xcc_ok, last = [], True, None
    for _ in range(reps + 3):
        C.probe_ramp(out, threads, lds)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        skews.append(float((o[:, 0].max() - o[:, 0].min()) * 0.01))
        xcc_ok &= bool(((o[:, 1] >> 16) == np.arange(blocks) % 8).all())
        last = o
    skews = skews[3:]  # the first launches load the code object
    per_xcd = [float(((last[np.arange(blocks) % 8 == x, 0]).max() - last[:, 0].min()) * 0.01) for x in range(8)]
    return {"threads": threads, "lds": lds, "skew_us_median": float(np.median(skews)), "skew_us_min": min(skews),
            "skew_us_max": max(skews), "xcc_is_block_mod_8": xcc_ok, "last_entry_by_xcd_us": per_xcd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from multidisttorch_amd.ops import native

    native.require()
    import multidisttorch_amd._C as C

    maps = step_map(a.batch, a.steps)
    print_step_map(maps[-1], a.batch)
    print("  first entry -> last entry per step:", " ".join(f"{max(m['start_us']):.2f}" for m in maps))
    rows = []
    print(f"\nempty kernel, {2 * a.batch} workgroups, entry skew over {a.reps} launches (us):")
    for threads, lds in ((512, STEP_LDS), (512, 65536), (512, 0), (256, STEP_LDS), (256, 65536), (256, 0)):
        r = probe(C, 2 * a.batch, threads, lds, a.reps)
        rows.append(r)
        print(f"  threads {threads:3d}  LDS {lds:6d} B: median {r['skew_us_median']:5.2f}  "
              f"min {r['skew_us_min']:5.2f}  max {r['skew_us_max']:5.2f}  XCC id == block % 8: {r['xcc_is_block_mod_8']}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"step": maps, "probe": rows}, f)


if __name__ == "__main__":
    main()
