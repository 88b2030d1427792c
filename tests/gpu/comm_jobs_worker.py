"""Worker of tests/gpu/test_comm_jobs_values.py::test_jobs_across_processes_every_form:
s processes share the MI355X (each confined to its own CU share,
MDT_CU_SPLIT=1) and run the fused all-reduce jobs (csrc/kernels/comm_jobs.h)
on the synthetic arena of tests/comm_checker.py, every rank with its own
gradients, in the forms that need concurrent peers:

  one-shot push+reduce (mode 3) | one-shot push, host barrier, reduce |
  two-shot push, host barrier, reduce | two-shot push+reduce

each without and with Adam, each on both receive parities. The one-shot forms
use the reducer's production descriptor (``comm_ctx()``: epoch = step + the
base the construction-time self-test left), the two-shot forms
``selftest_ctx(timeout, True)`` of the same reducer (base 0). The flags are
shared by every descriptor of a reducer and only grow, so the epochs increase
strictly over the whole run and start above the self-test's.

Every rank forms the expected values itself from the (rank, data) seeds and
checks its own arenas: bitwise ``reduce_ref``, Adam within ``adam_ref``'s
bounds. After any non-zero status (the ranks agree on that over gloo) nothing
more is launched.

prints one line ``RESULT <json>`` per rank.
"""
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

FORMS = [("one-shot push+reduce", False, False), ("one-shot push|barrier|reduce", False, True),
         ("two-shot push|barrier|reduce", True, True), ("two-shot push+reduce", True, False)]
FIRST_EPOCH = 8      # above the self-test's epochs (1, 2) and the base it leaves (<= 4)
UNIT_BYTES = 12


def main():
    from multidisttorch_amd.runtime.env import apply_cu_split

    apply_cu_split()  # disjoint CU shares per rank (before HIP initialises)
    dist.init_process_group("gloo")
    r, s = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    timeout_s = float(os.environ.setdefault("MDT_P2P_TIMEOUT_S", "10"))
    from multidisttorch_amd.ops import native
    from multidisttorch_amd.parallel.ddp import make_arena_reducer
    from tests import comm_checker as cc
    from tests import conv_small_checker as ck

    C = native.require()
    hp = ck.ADAM_SETS["coupled"]
    G = torch.full((cc.NUMEL,), cc.POISON, device=dev)
    P, m, v = (torch.zeros(cc.NUMEL, device=dev) for _ in range(3))
    w16 = torch.full((cc.NUMEL,), ck.BF16_FILL, dtype=cc.BF16, device=dev)
    slabs = {si: torch.zeros(ns, n, device=dev) for si, (_, n, ns) in enumerate(cc.SEGS) if ns}
    segs = C.make_grad_segs([[off, n, slabs[si].data_ptr() if ns else 0, max(ns, 1), 0, 0, 0, 0, -1]
                             for si, (off, n, ns) in enumerate(cc.SEGS)], 0)
    units = C.make_grad_units([list(u) for u in cc.UNITS], 0)
    nu = len(cc.UNITS)
    state = C.TrialState(0)
    state.set_hparams(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], 1.0, hp["grad_scale"], 0,
                      hp["decoupled"], lr_warmup_steps=hp["lr_warmup_steps"])

    red = make_arena_reducer(dist.group.WORLD, G, [0, cc.NUMEL], kind="xgmi")
    res = dict(rank=r, reducer=type(red).__name__, fails=[], runs=[], ratios={}, status=0, stopped=False)
    if not (hasattr(red, "fused") and red.fused()):
        res["fails"].append("no fused xGMI reducer (peer mapping or self-test failed)")
        print("RESULT " + json.dumps(res), flush=True)
        dist.destroy_process_group()
        return 1
    scale = red.scale()
    base = int(red.epoch_base())
    assert base < FIRST_EPOCH
    ctx1, ctx2 = red.comm_ctx(), red.selftest_ctx(timeout_s, True)
    packs = []

    def launch(ctx, mode, adam):
        job = C.Job()
        C.comm_job(P, G, m, v, w16, segs, units, nu, state.train_state, state.hparams, adam, ctx, mode, job)
        pack, grid = C.pack_jobs_multi([job])
        packs.append(pack.to(dev))
        C.launch_jobs_multi(packs[-1], grid)

    def agree_status(st):
        t = torch.tensor([st], dtype=torch.int64)
        out = [torch.empty_like(t) for _ in range(s)]
        dist.all_gather(out, t)
        return [int(o.item()) for o in out]

    epoch, k = FIRST_EPOCH, 0
    for name, two, split in FORMS:
        for adam in (False, True):
            for _ in range(2):                       # consecutive epochs: both parities
                data = 1 + k % 4                     # fresh (rank, data) inputs against the slot's previous use
                k += 1
                step = epoch if two else epoch - base
                G0, sl = cc.rank_data(r, data)
                G.copy_(G0)
                for si, t in sl.items():
                    slabs[si].copy_(t)
                p0, m0, v0 = cc.adam_state(data)
                for dst, src in zip((P, m, v), (p0, m0, v0)):
                    dst.copy_(src)
                w16.fill_(ck.BF16_FILL)
                state.set_step(False, step)
                ctx = ctx2 if two else ctx1
                torch.cuda.synchronize()
                dist.barrier()                       # every rank loaded its inputs and read its last results
                if split:
                    launch(ctx, 1, adam)
                    torch.cuda.synchronize()
                    dist.barrier()
                    launch(ctx, 2, adam)
                else:
                    launch(ctx, 3, adam)
                torch.cuda.synchronize()
                st = int(red.selftest_status(ctx2)) or int(red.status())
                all_st = agree_status(st)
                res["runs"].append([name, int(adam), epoch & 1])
                if any(all_st):
                    res["status"], res["stopped"] = st, True
                    res["fails"].append(f"{name} adam={adam} epoch {epoch}: status per rank {all_st}")
                    break
                own, want = cc.expected(s, data, scale)
                if not adam:
                    fails = cc.check_reduce(G.cpu(), want)
                else:
                    fails, ratios = cc.check_adam(P.cpu(), G.cpu(), m.cpu(), v.cpu(), w16.cpu(), own[r], want, p0, m0,
                                                  v0, ck.adam_consts(hp, step))
                    for key, val in ratios.items():
                        res["ratios"][key] = max(res["ratios"].get(key, 0.0), val)
                res["fails"] += [f"{name} adam={adam} epoch {epoch} (parity {epoch & 1}): {f}" for f in fails]
                packs.clear()
                epoch += 1
            if res["stopped"]:
                break
        if res["stopped"]:
            break
    torch.cuda.synchronize()
    dist.barrier()  # peers stop writing into our region before it is freed
    del red
    torch.cuda.synchronize()
    dist.barrier()
    print("RESULT " + json.dumps(res), flush=True)
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
