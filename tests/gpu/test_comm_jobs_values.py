"""The fused all-reduce jobs (csrc/kernels/comm_jobs.h, ``comm_unit_body``)
with more than one rank holding DIFFERENT gradients, per element against
tests/comm_checker.py: the push is bitwise the finalize order (``own_sum``),
the reduce bitwise the rank-order float32 sum x scale (``reduce_ref``), Adam
in the reduce's epilogue within ``adam_ref``'s own bounds on the expected
gradient. tests/unit/test_comm_checker.py shows on the CPU that this checker
fails a wrong peer slot, a dropped or doubled rank, a reversed order, a
pre-scaled sum, a stale parity slot, wrong two-shot chunks and an Adam fed the
own gradient.

Part A (this process): s reducers on the one device mapped to each other
(``connect_local``), one-shot, the jobs issued as ``selftest_fused`` issues
them. Every rank's push is launched before any reduce, so no job ever waits
for a producer queued behind it on the stream; a mistake here would end as a
status word after the reducers' 2 s bound, never as a hang.

Part B (tests/gpu/comm_jobs_worker.py): the same arena across s = 3, 4
processes: push+reduce in one workgroup and the two-shot form, which need
their peers to run concurrently.
"""
import json
import os
import sys

import pytest
import torch

from tests import comm_checker as cc
from tests import conv_small_checker as ck

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEV = torch.device("cuda", 0)
UNIT_BYTES = 12          # one GradUnit row (3 int32) of the uint8 unit table
TIMEOUT_S = 2.0
SEEN = {}                # largest Adam error / bound per stage, printed for the record


class _Rank:
    """One in-process rank: its arenas, slabs, segment table, state and reducer."""

    def __init__(self, C, r, s, hp):
        self.C, self.r = C, r
        self.G = torch.full((cc.NUMEL,), cc.POISON, device=DEV)
        self.P, self.m, self.v = (torch.zeros(cc.NUMEL, device=DEV) for _ in range(3))
        self.w16 = torch.full((cc.NUMEL,), ck.BF16_FILL, dtype=cc.BF16, device=DEV)
        self.slabs = {si: torch.zeros(ns, n, device=DEV) for si, (_, n, ns) in enumerate(cc.SEGS) if ns}
        self.segs = C.make_grad_segs([[off, n, self.slabs[si].data_ptr() if ns else 0, max(ns, 1), 0, 0, 0, 0, -1]
                                      for si, (off, n, ns) in enumerate(cc.SEGS)], 0)
        hp = hp or ck.ADAM_SETS["default"]
        self.state = C.TrialState(0)
        self.state.set_hparams(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], 1.0,
                               hp["grad_scale"], 0, hp["decoupled"], lr_warmup_steps=hp["lr_warmup_steps"])
        self.red = C.XgmiP2PReducer(r, s, self.G, [0, cc.NUMEL], True, 0.0, 64, TIMEOUT_S, -1, True)
        self.packs = []      # device job tables stay alive until the launches that read them have run

    def load(self, epoch, adam):
        G0, slabs = cc.rank_data(self.r, epoch)
        self.G.copy_(G0)
        for si, t in slabs.items():
            self.slabs[si].copy_(t)
        if adam:
            for dst, src in zip((self.P, self.m, self.v), cc.adam_state(epoch)):
                dst.copy_(src)
            self.w16.fill_(ck.BF16_FILL)
        self.state.set_step(False, epoch)     # the jobs' epoch (ctx ep_base 0) and Adam's step

    def launch(self, units, mode, adam, split=None):
        """One launch of the jobs over all units (``split``: as two jobs in the
        one launch, units [0, split) and [split, n), as the step's tails do)."""
        C, n = self.C, len(cc.UNITS)
        jobs = []
        for u0, u1 in ([(0, n)] if split is None else [(0, split), (split, n)]):
            job = C.Job()
            C.comm_job(self.P, self.G, self.m, self.v, self.w16, self.segs,
                       units.narrow(0, u0 * UNIT_BYTES, (u1 - u0) * UNIT_BYTES), u1 - u0, self.state.train_state,
                       self.state.hparams, bool(adam), self.red.comm_ctx(), mode, job)
            jobs.append(job)
        pack, grid = C.pack_jobs_multi(jobs)
        assert grid == n
        self.packs.append(pack.to(DEV))
        C.launch_jobs_multi(self.packs[-1], grid)


def _ranks(C, s, hp=None):
    ranks = [_Rank(C, r, s, hp) for r in range(s)]
    bases = [k.red.local_base() for k in ranks]
    for k in ranks:
        k.red.connect_local(bases)
    units = C.make_grad_units([list(u) for u in cc.UNITS], 0)
    return ranks, units


def _ok(name, r):
    SEEN[name] = max(SEEN.get(name, 0.0), r)
    print(f"RATIO {name} {r:.4g}")


@pytest.mark.parametrize("adam", [None, "coupled", "decoupled"])
@pytest.mark.parametrize("s", [2, 3, 5, 8])
def test_one_shot_jobs_reduce_rank_distinct_gradients(native_ext, s, adam):
    C = native_ext
    hp = ck.ADAM_SETS[adam] if adam else None
    ranks, units = _ranks(C, s, hp)
    scale = ranks[0].red.scale()
    assert scale == float(torch.tensor(1.0 / s, dtype=torch.float32))
    for e in cc.EPOCHS:                       # both parities twice, fresh data every epoch
        own, red = cc.expected(s, e, scale)
        for k in ranks:
            k.load(e, adam)
        split = 7 if e == 2 else None         # epoch 2: two jobs in one launch
        for k in ranks:
            k.launch(units, 1, adam, split)
        if e == 3:
            torch.cuda.synchronize()
            for k in ranks:
                assert cc.check_push(k.G.cpu(), own[k.r]) == [], (s, e, k.r)
        for k in ranks:
            k.launch(units, 2, adam, split)
        torch.cuda.synchronize()
        status = [int(k.red.status()) for k in ranks]
        assert status == [0] * s, (s, e, status)
        for k in ranks:
            if not adam:
                fails = cc.check_reduce(k.G.cpu(), red)
            else:
                p0, m0, v0 = cc.adam_state(e)
                fails, ratios = cc.check_adam(k.P.cpu(), k.G.cpu(), k.m.cpu(), k.v.cpu(), k.w16.cpu(), own[k.r], red,
                                              p0, m0, v0, ck.adam_consts(hp, e))
                for name, r in ratios.items():
                    _ok(f"comm_adam.{adam}.{name}", r)
            assert fails == [], (s, e, k.r, fails)
        for k in ranks:
            k.packs.clear()


def test_fused_reducer_of_a_group_rejects_an_arena_outside_the_domain(native_ext):
    """numel a multiple of 4 is the domain of the jobs' 16-B stores into a
    peer's [parity][src][numel] slots; both trainers' arenas are 64-aligned
    and nothing builds a fused reducer of a group on another arena, so the
    constructor refuses one (host side: nothing is launched)."""
    C = native_ext
    G = torch.zeros(1002, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        C.XgmiP2PReducer(0, 2, G, [0, 1002], True, 0.0, 64, TIMEOUT_S, -1, True)
    C.XgmiP2PReducer(0, 1, G, [0, 1002], True, 0.0, 64, TIMEOUT_S, -1, True)    # one rank: nothing to store
    C.XgmiP2PReducer(0, 2, G, [0, 1002], True, 0.0, 64, TIMEOUT_S, -1, False)   # the bucket kernels take any size


# ------------------------------------------------ part B: across processes ----
FORMS = ["one-shot push+reduce", "one-shot push|barrier|reduce", "two-shot push|barrier|reduce",
         "two-shot push+reduce"]


@pytest.mark.parametrize("s", [3, 4])
def test_jobs_across_processes_every_form(s):
    from multidisttorch_amd.launch import launch

    env = {"PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2", "MDT_CU_SPLIT": "1", "MDT_P2P_TIMEOUT_S": "10"}
    rc, outs = launch([sys.executable, os.path.join(HERE, "comm_jobs_worker.py")], s, emulate="torchrun", timeout=150,
                      extra_env=env, capture=True)
    text = "\n".join(o or "" for o in outs)
    res = [json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT ")]
    assert rc == 0 and len(res) == s, text[-4000:]
    for r in res:
        assert r["fails"] == [], r
        assert r["status"] == 0 and not r["stopped"], r
        # every form, with and without Adam, on both parities
        assert sorted(r["runs"]) == sorted([f, a, p] for f in FORMS for a in (0, 1) for p in (0, 1)), r
        for name, v in r["ratios"].items():
            _ok(f"comm_adam.procs{s}.{name}", v)


# --------------------------- part C: the real step, rank-distinct gradients ----
# one launch per (group, reducer kind, models): the 128x128 model gets a launch of its own, so that no launch
# takes more than 1.5 times the slowest test_conv_p2p_multiprocess_ddp case of its group size
STEP_LAUNCHES = [(s, kind, models) for s, kind in [(2, "xgmi"), (3, "xgmi1"), (3, "xgmi2"), (4, "xgmi2")]
                 for models in ("f28,layer28", "layer128")]


@pytest.mark.parametrize("s,kind,models", STEP_LAUNCHES)
def test_real_step_reduces_rank_distinct_gradients(s, kind, models):
    """tests/gpu/comm_step_worker.py: every rank trains on its own rows and
    noise stream; ``tr.grads`` must be ``reduce_ref`` of the ranks' own
    contributions (twin trainers with a one-rank fused reducer) bitwise, Adam
    on the expected gradient within ``adam_ref``'s bounds, graph replay bitwise
    the value-checked eager steps. CU-split ranks with the paired 28x28 kernel
    off: which partner pairs is a race, so a twin need not agree bit for bit
    with it on (the paired form keeps its replica-equality tests)."""
    from multidisttorch_amd.launch import launch

    env = {"PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2", "MDT_CU_SPLIT": "1", "MDT_F28_PAIR": "0",
           "MDT_P2P_TIMEOUT_S": "20"}
    rc, outs = launch([sys.executable, os.path.join(HERE, "comm_step_worker.py"), kind, models], s,
                      emulate="torchrun", timeout=150, extra_env=env, capture=True)
    text = "\n".join(o or "" for o in outs)
    print("\n".join(l for l in text.splitlines() if l.startswith(("PLAN ", "RATIO "))))
    res = [json.loads(l[7:]) for l in text.splitlines() if l.startswith("RESULT ")]
    assert rc == 0 and len(res) == s, text[-4000:]
    for r in res:
        assert r["fails"] == [] and not r["stopped"], (r["rank"], r["fails"])
        assert r["cu_mask"] and r["pair"] == "0", r
        assert sorted(r["models"]) == sorted(models.split(",")), r
        for name, info in r["models"].items():
            assert info["steps"] == 5 and set(info["adam"]) >= {"AD.params", "AD.exp_avg", "AD.exp_avg_sq", "AD.w16"}
            assert all(v <= 1 for v in info["adam"].values()), (name, info["adam"])
            for key, val in info["adam"].items():
                SEEN[f"comm_step.{name}.{key}"] = max(SEEN.get(f"comm_step.{name}.{key}", 0.0), val)
    print("worker seconds per model (rank 0):",
          {n: i["total_s"] for n, i in [r for r in res if r["rank"] == 0][0]["models"].items()})


def test_report_largest_adam_ratios():
    """Not a check of its own: the largest Adam error / bound per stage over the module's run, for the record."""
    for name in sorted(SEEN):
        print(f"MAX {name} {SEEN[name]:.4g}")
    assert all(v <= 1 for v in SEEN.values())
