"""Worker of tests/gpu/test_comm_jobs_values.py::test_real_step_reduces_rank_distinct_gradients:
s CU-split processes share the MI355X and train conv-VAE trials data-parallel
through the fused xGMI reducer (csrc/kernels/comm_jobs.h as jobs of the step's
own launches), every rank on ITS OWN rows and noise stream, so the s
contributions differ in every element.

Per model (fused 28x28 z = 32 B = 8; layer path 28x28 z = 24 B = 16; layer
path 128x128 z = 64 B = 8):

  values   four eager steps without Adam (``f28_skip_adam`` /
           ``comm_skip_adam``), M = B, 5, B, 5: another unit decomposition of
           the same arena per step, each parity slot reused. A twin trainer
           with a ONE-rank fused reducer (scale 1) runs the same launches and
           jobs with nothing to move: its gradient arena is this rank's own
           contribution. The ranks all-gather the twins' arenas over gloo, and
           ``tr.grads`` must equal ``comm_checker.reduce_ref`` of them bitwise.
  Adam     a fresh DDP trainer with moments planted equally on every rank,
           first step: ``knob_cases.check_adam`` on the expected gradient, the
           bf16 twin, the arena still the own contribution, the transposed
           weight copies after ``_ensure_wt``.
  graphs   that trainer goes on eagerly to five steps (the last a tail); a
           second one replays graphs (``graph_steps = 2``) from the same start:
           parameters, both moments and the loss ring bitwise equal.

After any non-zero status nothing more is launched (the ranks agree on that
over gloo). argv: reducer kind [models, comma-separated: the test gives the
128x128 model a launch of its own]. Prints one line ``RESULT <json>`` per rank.
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, image, z, B, fused 28x28 step)
MODELS = [("f28", 28, 32, 8, True), ("layer28", 28, 24, 16, False), ("layer128", 128, 64, 8, False)]
NB, TAIL = 4, 5
U = 2.0 ** -24


class Stop(Exception):
    pass


def main():
    kind = sys.argv[1]
    only = sys.argv[2].split(",") if len(sys.argv) > 2 else None
    from multidisttorch_amd.runtime.env import apply_cu_split

    apply_cu_split()  # disjoint CU shares per rank (before HIP initialises)
    dist.init_process_group("gloo")
    r, s = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    os.environ.setdefault("MDT_P2P_TIMEOUT_S", "20")
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.parallel.ddp import SELFTEST_LOG, broadcast_params, make_arena_reducer
    from tests import comm_checker as cc
    from tests import conv_small_checker as ck
    from tests import knob_cases as kc
    from tests import layer_checker as lk
    from tests.gpu import test_conv_layer_stages as ls

    res = dict(rank=r, kind=kind, fails=[], stopped=False, models={}, pair=os.environ.get("MDT_F28_PAIR"),
               cu_mask=os.environ.get("HSA_CU_MASK"))
    fails = res["fails"]

    def gather(t):
        out = [torch.empty_like(t) for _ in range(s)]
        dist.all_gather(out, t)
        return out

    def agree_ok(tr, where):
        """status() and f28_err of this rank's DDP trainer; every rank stops when any is non-zero."""
        st = int(tr.reducer.status())
        err = int(tr.f28_err.item()) if tr.f28 else 0
        all_st = [tuple(x.tolist()) for x in gather(torch.tensor([st, err], dtype=torch.int64))]
        if any(a != (0, 0) for a in all_st):
            fails.append(f"{where}: (status, f28_err) per rank {all_st}")
            res["stopped"] = True
            raise Stop()

    def drop(tr):
        torch.cuda.synchronize()
        dist.barrier()  # peers stop writing into our region before it is freed
        tr.attach_reducer(None)  # also drops the graphs that reference the peer regions
        torch.cuda.synchronize()
        dist.barrier()

    def run_model(name, image, z, B, f28):
        t0 = time.time()
        info = res["models"][name] = {}
        D = image * image
        rows = NB * B
        X = torch.rand(s * rows, D, generator=torch.Generator().manual_seed(11)).to(dev)
        idx = torch.arange(r * rows, (r + 1) * rows, device=dev, dtype=torch.int32)   # this rank's own rows

        def make(graphs=False, skip=False):
            tr = ConvVaeTrainer(batch_size=B, image=image, z=z, device=dev, backend="hip", seed=7, init_seed=7 + r,
                                lr=2e-3, rng_stream=r, use_graphs=graphs, graph_steps=2)
            assert tr.f28 == f28
            tr.f28_skip_adam = tr.comm_skip_adam = skip
            return tr

        def start(tr, params, ddp):
            with torch.no_grad():
                tr.params.copy_(params)
            tr.refresh_weights()
            if ddp:
                n_log = len(SELFTEST_LOG)
                red = make_arena_reducer(dist.group.WORLD, tr.grads, tr.bucket_bounds(None), kind=kind)
                assert type(red).__name__ == "XgmiP2PReducer" and red.fused(), type(red).__name__
                assert bool(red.fused_two_shot()) == (kind == "xgmi2" and s > 2)
                assert len(SELFTEST_LOG) > n_log and SELFTEST_LOG[-1]["result"] == "ok", SELFTEST_LOG[-1:]
            else:   # the twin: one rank, scale 1, the same jobs with nothing to move
                red = tr.C.XgmiP2PReducer(0, 1, tr.grads, tr.default_bucket_bounds(), True, 1.0, 64, 20.0, -1, True)
            tr.attach_reducer(red)
            tr.bind_train_data(X, idx)
            tr.set_cursor(0, NB)
            return red

        def classes(tr, M):
            p = tr._plan28(M) if f28 else tr._plan(M)
            cnt = p["units"].cpu().view(torch.int32).reshape(-1, 3)[: p["nunits"], 2]
            small, vec4 = int((cnt <= 256).sum()), int((cnt > 256).sum())
            slabbed = sorted(k for k in p["slabs"])
            free = sorted(n for n, _, _ in tr.layout if n not in p["slabs"])
            print(f"PLAN {name} M={M}: {small} small units (count <= 256), {vec4} vec4 units, "
                  f"{len(slabbed)} slab-summed segments, {len(free)} slab-free segments {free}", flush=True)
            info[f"classes_M{M}"] = [small, vec4, len(slabbed), len(free)]
            if not (small and vec4):
                fails.append(f"{name} M={M}: the plan lacks a unit class (small {small}, vec4 {vec4})")

        # ---------------------------------------------------------- values ----
        tr = make(skip=True)
        broadcast_params([tr.params], dist.group.WORLD)   # the replicas start from rank 0's weights
        params0 = tr.params.clone()
        red = start(tr, params0, True)
        scale = red.scale()
        tw = make(skip=True)
        start(tw, params0, False)
        for M in (B, TAIL):
            classes(tr, M)
        segs = [(n, o, int(np.prod(sh))) for n, o, sh in tr.layout]
        for k, M in enumerate((B, TAIL, B, TAIL)):
            tw.train_steps(1, M=M)
            torch.cuda.synchronize()
            own = tw.grads.cpu()
            tr.train_steps(1, M=M)
            torch.cuda.synchronize()
            agree_ok(tr, f"{name} values step {k}")
            got = tr.grads.cpu()
            owns = gather(own)
            want = cc.reduce_ref(owns, scale)
            where = f"{name} step {k} (M={M}, epoch parity {(k + 1 + int(red.epoch_base())) & 1})"
            if not torch.equal(got, want):
                mag = sum(o.abs() for o in owns).double()
                bound = (s + 2) * U * scale * mag
                err = (got.double() - want.double()).abs()
                bad = {n: int((got[o:o + c] != want[o:o + c]).sum()) for n, o, c in segs}
                # which side moves: the twin run again from the same state must repeat itself
                tw.set_step(k)
                tw.set_cursor(k % NB, NB)
                tw.train_steps(1, M=M)
                torch.cuda.synchronize()
                fails.append(f"{where}: grads differ from reduce_ref in {({n: b for n, b in bad.items() if b})}; "
                             f"largest error / ((s + 2) u scale sum|g|) "
                             f"{float((err / bound.clamp_min(1e-300)).max()):.3g}; "
                             f"twin repeats itself: {bool(torch.equal(tw.grads.cpu(), own))}")
            if not bool(torch.isfinite(got).all()):
                fails.append(f"{where}: non-finite gradient")
            # the inputs make a wrong reduce visible
            for n, o, c in segs:
                if c <= 16:
                    continue
                nz = torch.zeros(c, dtype=torch.bool)
                for g in owns:
                    nz |= g[o:o + c] != 0
                for q, g in enumerate(owns):
                    share = float((want[o:o + c][nz] != g[o:o + c][nz]).double().mean()) if bool(nz.any()) else 0.0
                    if share < 0.5:
                        fails.append(f"{where}: {n}: the expected value equals rank {q}'s own contribution in "
                                     f"{1 - share:.2f} of the non-zero elements")
            if s >= 3 and torch.equal(cc.reverse_ref(owns, scale), got):
                fails.append(f"{where}: the reverse-order sum reproduces the result (order not visible)")
            if not torch.equal(tr.params, params0):
                fails.append(f"{where}: parameters moved without Adam")
        info["values_s"] = round(time.time() - t0, 2)
        drop(tr)
        del tr, red

        # ------------------------------------------------ Adam, first step ----
        tA = make()
        redA = start(tA, params0, True)
        kc.plant_optimizer_state(tA)
        tw.set_step(0)
        tw.set_cursor(0, NB)
        tw.train_steps(1, M=B)
        torch.cuda.synchronize()
        own = tw.grads.cpu()
        want = cc.reduce_ref(gather(own), scale)
        before = dict(params=tA.params.clone(), exp_avg=tA.exp_avg.clone(), exp_avg_sq=tA.exp_avg_sq.clone())
        tA.train_steps(1, M=B)
        torch.cuda.synchronize()
        agree_ok(tA, f"{name} Adam step")
        after = dict(params=tA.params.clone(), exp_avg=tA.exp_avg.clone(), exp_avg_sq=tA.exp_avg_sq.clone(),
                     w16=tA.w16.clone())
        c = ck.adam_consts(lk.adam_hp(tA.hp, tA.decoupled_wd, tA.schedule), 1)
        ratios = kc.check_adam(before, after, want, c)
        info["adam"] = ratios
        for key, val in ratios.items():
            print(f"RATIO comm_step.{name}.{key} {val:.4g}", flush=True)
            if not val <= 1:
                fails.append(f"{name} Adam on the expected gradient: {key} error / bound {val:.4g}")
        if torch.equal(after["params"], before["params"]):
            fails.append(f"{name}: Adam did not move the parameters")
        if not torch.equal(tA.grads.cpu(), own):
            fails.append(f"{name} Adam step: the arena does not hold the own contribution (the twin's)")
        tA._ensure_wt()
        torch.cuda.synchronize()
        try:
            ls._check_wt(tA, tA.w16)
        except AssertionError as e:
            fails.append(f"{name}: transposed weight copy of {e} is not the parity transpose of w16")
        info["adam_s"] = round(time.time() - t0, 2)

        # ------------------------------------- graphs against eager, 5 steps ----
        tA.train_steps(3)
        tA.train_steps(1, M=TAIL)
        torch.cuda.synchronize()
        agree_ok(tA, f"{name} eager steps")
        eager = [t.cpu() for t in (tA.params, tA.exp_avg, tA.exp_avg_sq)] + [tA.loss_history()[:5].copy()]
        drop(tA)
        del tA, redA
        tG = make(graphs=True)
        redG = start(tG, params0, True)
        kc.plant_optimizer_state(tG)
        assert tG.use_graphs
        tG.train_steps(4)
        tG.train_steps(1, M=TAIL)
        torch.cuda.synchronize()
        agree_ok(tG, f"{name} graph steps")
        graph = [t.cpu() for t in (tG.params, tG.exp_avg, tG.exp_avg_sq)] + [tG.loss_history()[:5].copy()]
        for what, a, b in zip(("params", "exp_avg", "exp_avg_sq"), eager, graph):
            if not torch.equal(a, b):
                fails.append(f"{name}: {what} after 5 steps differ between eager and graph replay "
                             f"(max {float((a - b).abs().max()):.3g})")
        if not np.array_equal(eager[3], graph[3]) or not np.isfinite(graph[3]).all():
            fails.append(f"{name}: loss ring differs between eager and graph replay: {eager[3]} {graph[3]}")
        info["steps"] = int(tG.read_state()["step"])
        drop(tG)
        del tG, redG
        tw.attach_reducer(None)
        info["total_s"] = round(time.time() - t0, 2)

    try:
        for m in MODELS:
            if only is None or m[0] in only:
                run_model(*m)
    except Stop:
        pass
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
