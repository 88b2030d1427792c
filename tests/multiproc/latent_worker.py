"""Worker of tests/multiproc/test_latent_multiproc.py: one trial with
``latent_report`` on a single group spanning the world; every member prints
``RESULT <json>`` with the report it computed.
"""
import faulthandler
import json
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch.distributed as dist  # noqa: E402


def main():
    from multidisttorch_amd.hpo.runner import RunOptions, run_trial
    from multidisttorch_amd.hpo.trial import build_specs
    from multidisttorch_amd.parallel.groups import setup_ddp_groups
    from multidisttorch_amd.runtime.bootstrap import control_group, global_barrier, setup_ddp, shutdown
    from multidisttorch_amd.runtime.faults import create_health_groups

    _, rank = setup_ddp(verbose=False)
    groups = setup_ddp_groups(1)
    control_group()
    create_health_groups(1)
    spec = build_specs(1, 1, None, None, 3)[0]
    opts = RunOptions(batch_size=32, backend="torch", results=False, train_samples=256, test_samples=85,
                      synthetic=True, model=sys.argv[1], latent_report=True)
    res = run_trial(spec, groups[0], opts)
    lat = dict(res.extra.get("latent", {}))
    lat.pop("latent_s", None)
    print("RESULT " + json.dumps(dict(rank=rank, grank=dist.get_rank(groups[0]), failed=res.failed, latent=lat)),
          flush=True)
    global_barrier()
    shutdown()


if __name__ == "__main__":
    main()
