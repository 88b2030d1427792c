"""Worker of tests/gpu/test_ema_gpu.py::test_two_replicas_hold_bitwise_equal_averages:
two processes share the MI355X (each confined to its own CU share, MDT_CU_SPLIT=1)
and train one 28x28 conv-VAE trial data-parallel through the fused xGMI reducer,
whose all-reduce runs as jobs of the step's own launches (csrc/kernels/comm_jobs.h),
with a weight average: the shipped form (graph replay, the in-kernel wait). The
order of the launch-issuing calls is recorded while the first step graph is
captured: the step's last two must be the comm-job tail and ``ema_update``.

argv: decay -> prints one line ``RESULT <json>`` per rank.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


class _CallLog:
    """Proxy of the native module recording the order of launch-issuing calls."""

    def __init__(self, C, log):
        self._C, self._log = C, log

    def __getattr__(self, name):
        f = getattr(self._C, name)
        if not callable(f) or name[0].isupper():
            return f

        def wrap(*a, **k):
            self._log.append(name)
            return f(*a, **k)

        return wrap


def main():
    decay = float(sys.argv[1])
    from multidisttorch_amd.runtime.env import apply_cu_split

    apply_cu_split()  # disjoint CU shares per rank (before HIP initialises)
    dist.init_process_group("gloo")
    r, s = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    os.environ["MDT_P2P_TIMEOUT_S"] = "20"
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.parallel.ddp import broadcast_params, make_arena_reducer

    B, nb, tail = 8, 4, 5
    n = nb * B + tail
    X = torch.rand(n, 784, generator=torch.Generator().manual_seed(11)).to(dev)
    idx = torch.arange(n, device=dev, dtype=torch.int32)
    tr = ConvVaeTrainer(batch_size=B, image=28, z=32, device=dev, backend="hip", seed=7, init_seed=7 + r, lr=3e-3,
                        rng_stream=r, use_graphs=True, graph_steps=2, ema_decay=decay)
    broadcast_params([tr.params], dist.group.WORLD)  # the replicas start from rank 0's weights ...
    tr.refresh_weights()
    tr.reset_average()                               # ... and so do their averages
    red = make_arena_reducer(dist.group.WORLD, tr.grads, tr.bucket_bounds(None), kind="xgmi")
    tr.attach_reducer(red)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, nb + 1)

    log = []
    tr.C = _CallLog(tr.C, log)
    ema_step = tr._ema_step_hip

    def logged_ema_step():
        log.append("ema_update")
        ema_step()

    tr._ema_step_hip = logged_ema_step
    tr.train_steps(1)
    # warm-up step + captured step; the capture is followed by a cast of the restored weights: the
    # step ends at its ema_update
    first = log[: len(log) - log[::-1].index("ema_update")]
    tr.train_steps(nb - 1)
    tr.train_steps(1, M=tail)
    tr.train_steps(1)
    torch.cuda.synchronize()

    def same(t):
        out = [torch.empty_like(t) for _ in range(s)]
        dist.all_gather(out, t)
        return all(torch.equal(out[0], o) for o in out)

    steps = nb + 2
    res = dict(rank=r, reducer=type(red).__name__, fused=bool(red.fused()) if hasattr(red, "fused") else False,
               status=int(red.status()) if hasattr(red, "status") else 0, tail=first[-2:], calls=first,
               params_equal=same(tr.params.cpu()), ema_equal=same(tr.ema.cpu()),
               moved=not torch.equal(tr.ema, tr.params), step=tr.read_state()["step"],
               finite=bool(torch.isfinite(tr.ema).all().item()),
               losses=tr.loss_history()[:steps].astype(np.float64).tolist())
    dist.barrier()  # peers stop writing into our region before it is freed
    tr.attach_reducer(None)
    del red, tr
    torch.cuda.synchronize()
    dist.barrier()
    print("RESULT " + json.dumps(res), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
