"""Worker of tests/multiproc/test_ema_multiproc.py: two replicas of one trial (a
group of 2, gloo, torch backend) that keep a weight average. The replicas
start from different initial weights; after the constructor broadcast the
average is reset to the shared ones. Prints one line ``RESULT <json>`` per rank."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
    from multidisttorch_amd.parallel.ddp import broadcast_params, make_arena_reducer
    from multidisttorch_amd.runtime.bootstrap import global_barrier, setup_ddp, shutdown

    ws, wr = setup_ddp(verbose=False)
    pg = dist.new_group(list(range(ws)))
    tr = MlpVaeTrainer(batch_size=32, D=64, H=32, Z=4, backend="torch", seed=3, init_seed=3 + wr, rng_stream=wr,
                       lr=3e-3, ema_decay=float(sys.argv[1]))
    broadcast_params([tr.params], pg)
    tr.refresh_weights()
    stale = not torch.equal(tr.ema, tr.params)  # rank 1's average still holds its own initial weights
    tr.reset_average()
    tr.attach_reducer(make_arena_reducer(pg, tr.grads, [0, tr.split, tr.numel]))
    X = torch.rand(256, 64, generator=torch.Generator().manual_seed(9))
    tr.bind_train_data(X, torch.arange(256, dtype=torch.int32))
    tr.set_cursor(0, 8)
    tr.train_steps(5)

    def same(t):
        out = [torch.zeros_like(t) for _ in range(ws)]
        dist.all_gather(out, t.clone())
        return all(torch.equal(a, out[0]) for a in out)

    print("RESULT " + json.dumps(dict(rank=wr, stale_before_reset=stale, params_equal=same(tr.params),
                                      ema_equal=same(tr.ema), moved=not torch.equal(tr.ema, tr.params),
                                      step=tr.read_state()["step"])), flush=True)
    global_barrier()
    shutdown()


if __name__ == "__main__":
    main()
