"""
Concurrent VAE hyper-parameter search over K process groups (MI355X-native).

Drop-in for /root/reference/vae-hpo.py: same flags and defaults
(``--batch-size 128 --epochs 3 --ngroups 2``), same stdout lines, same
``results-{group_rank}/`` images, same schedule (trial g trains epochs+g
epochs). Launch one process per GPU with any launcher the reference supports
(jsrun / srun / mpirun) or torchrun / ``python -m multidisttorch_amd.launch``.

Extensions (opt-in, default output unchanged): ``--lr`` / ``--beta`` (scalar or
comma list, one per trial), the per-trial schedules ``--lr-warmup`` / ``--lr-decay``
/ ``--lr-decay-steps`` / ``--lr-min-ratio`` / ``--kl-anneal`` (same form;
multidisttorch_amd/hpo/schedule.py), ``--free-bits`` (same form: a KL floor in nats
per sample and latent dimension, training only), ``--tc-weight`` (same form: the weight
of a minibatch total-correlation penalty in the training objective), ``--ema-decay`` (same
form: the decay of a weight average that every evaluation then uses), ``--seed``, ``--ckpt-dir`` + ``--resume``,
``--metrics-dir`` (JSONL + aggregate samples/s), ``--per-group-results``, ``--bucket-mb``,
``--no-graphs``, ``--backend {hip,torch}``, ``--synthetic/--real-data``,
``--trials-per-group T`` (T concurrent trials per single-rank group, one HIP
stream each: trial packing on MI355X), ``--iw-samples K`` (after each trial's
last epoch: the K-sample importance-weighted test log-likelihood, a score that
does not depend on the trial's beta), ``--latent-report`` (+ ``--au-threshold``;
after each trial's last epoch: active units and the MI / TC / dimension-wise-KL
split of the KL term over the test set), ``--binarize {none,threshold,static,dynamic}``
(train and test on {0, 1} pixels, redrawn on the device: the test loss and the
IW bound are then negative log-likelihoods of binarized data; one value per run),
``--sample-report N`` (after each trial's last epoch: the kernel MMD and the 1-NN
two-sample test between N decoded prior samples and N test rows).
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from utils import *  # noqa: F401,F403  (reference-compatible API + re-exports)

from multidisttorch_amd.data.binarize import BINARIZE_CHOICES
from multidisttorch_amd.hpo import objective
from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.runner import RunOptions, idle_rank, run_packed_trials, run_trial
from multidisttorch_amd.hpo.trial import build_specs, parse_list
from multidisttorch_amd.parallel.autotune import parse_bucket_mb
from multidisttorch_amd.runtime.bootstrap import control_group, global_barrier, shutdown
from multidisttorch_amd.runtime.faults import create_health_groups


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="VAE MNIST Example")
    parser.add_argument("--batch-size", type=int, default=128, metavar="N",
                        help="input batch size for training (default: 128)")
    parser.add_argument("--epochs", type=int, default=3, metavar="N",
                        help="number of epochs to train (default: 1)")
    parser.add_argument("--ngroups", type=int, help="number of groups", default=2)
    # ---- extensions ----
    parser.add_argument("--lr", type=str, default=None, help="learning rate(s), comma list per trial")
    parser.add_argument("--beta", type=str, default=None, help="KLD weight(s), comma list per trial")
    # per-trial schedules (hpo/schedule.py): a scalar or a comma list per trial, like --lr / --beta
    parser.add_argument("--lr-warmup", type=str, default=None, help="linear lr warm-up steps")
    parser.add_argument("--lr-decay", type=str, default=None, help="lr decay after the warm-up: none | cosine")
    parser.add_argument("--lr-decay-steps", type=str, default=None,
                        help="total steps of the lr schedule, warm-up included (default: the trial's step count)")
    parser.add_argument("--lr-min-ratio", type=str, default=None, help="cosine floor as a fraction of lr, in [0, 1]")
    parser.add_argument("--kl-anneal", type=str, default=None,
                        help="steps over which the KLD weight ramps linearly from 0 to --beta")
    for knob in objective.KNOBS:  # --free-bits, --tc-weight, --ema-decay: the same form (hpo/objective.py)
        parser.add_argument(knob.flag, type=str, default=None, help=knob.help)
    parser.add_argument("--seed", type=int, default=0, help="base seed (trial g uses seed+g)")
    parser.add_argument("--no-epoch-offset", action="store_true", help="all trials train --epochs epochs")
    parser.add_argument("--log-interval", type=int, default=10)
    parser.add_argument("--ckpt-dir", type=str, default=None)
    parser.add_argument("--resume", action="store_true")
    parser.add_argument("--metrics-dir", type=str, default=None)
    parser.add_argument("--per-group-results", action="store_true")
    parser.add_argument("--no-results", action="store_true", help="skip PNG writing")
    parser.add_argument("--no-graphs", action="store_true")
    parser.add_argument("--graph-steps", type=int, default=10)
    parser.add_argument("--backend", type=str, default=None, choices=[None, "hip", "torch"])
    parser.add_argument("--real-data", action="store_true", help="require MNIST IDX files under --data-dir")
    parser.add_argument("--synthetic", action="store_true",
                        help="always use the synthetic MNIST-shaped set (default: IDX files under --data-dir "
                             "or data-dir/MNIST/raw when present, synthetic otherwise)")
    parser.add_argument("--data-dir", type=str, default="data")
    parser.add_argument("--train-samples", type=int, default=None)
    parser.add_argument("--test-samples", type=int, default=None)
    parser.add_argument("--model", type=str, default="mlp", choices=["mlp", "conv"],
                        help="mlp = reference MLP-VAE (fp32); conv = bf16 conv/deconv VAE")
    parser.add_argument("--image-size", type=int, default=28, choices=[28, 128])
    parser.add_argument("--dtype", type=str, default=None, choices=[None, "fp32", "bf16"],
                        help="compute dtype; mlp runs fp32 (the reference's precision), conv runs bf16 MFMA")
    parser.add_argument("--profile", action="store_true",
                        help="roctx ranges around phases (rocprofv3 --marker-trace) + synced phase timings in metrics")
    parser.add_argument("--debug-sync", action="store_true",
                        help="serialize every kernel launch (AMD_SERIALIZE_KERNEL=3): race / fault triage")
    parser.add_argument("--trials-per-group", type=int, default=1,
                        help="train T trials concurrently per (single-rank) group, one HIP stream each")
    parser.add_argument("--bucket-mb", type=str, default=None,
                        help="intra-group all-reduce buckets: MiB cap, 0 = one bucket, 'auto' = measured")
    parser.add_argument("--iw-samples", type=int, default=0, metavar="K",
                        help="after each trial's last epoch: K-sample importance-weighted test log-likelihood "
                             "(a beta-independent score; 0 = off)")
    parser.add_argument("--latent-report", action="store_true",
                        help="after each trial's last epoch: KL per dimension, active units and the MI / TC / "
                             "dimension-wise-KL split of the KL term over the test set")
    parser.add_argument("--au-threshold", type=float, default=0.01,
                        help="a latent dimension is active when the variance of its posterior mean exceeds this")
    parser.add_argument("--binarize", type=str, default="none", choices=list(BINARIZE_CHOICES),
                        help="binarize the data on the device: threshold = x >= 0.5; static = one Bernoulli(x) draw "
                             "per trial; dynamic = a fresh draw of the training rows every epoch. The test set is "
                             "drawn once. One value for the whole run: trials of a sweep share a likelihood")
    parser.add_argument("--sample-report", type=int, default=0, metavar="N",
                        help="after each trial's last epoch: kernel MMD and 1-NN two-sample test between N decoded "
                             "prior samples and the first N test rows (a score of the samples themselves; 0 = off)")
    args = parser.parse_args(argv)
    if args.sample_report != 0:
        from multidisttorch_amd.models.sample_report import check_sample_args

        check_sample_args(args.sample_report, args.sample_report, 1)
        if args.test_samples is not None and args.sample_report > args.test_samples:
            raise ValueError(f"--sample-report {args.sample_report} exceeds --test-samples {args.test_samples}")
    return args


def main(argv=None):
    args = parse_args(argv)
    from multidisttorch_amd.runtime.env import apply_cu_split

    apply_cu_split()  # one-GPU multi-rank rehearsals only (MDT_CU_SPLIT=1), before HIP initialises
    if args.debug_sync:  # must precede any HIP initialisation
        os.environ["AMD_SERIALIZE_KERNEL"] = "3"
        os.environ["AMD_SERIALIZE_COPY"] = "3"
    want = {"mlp": "fp32", "conv": "bf16"}[args.model]
    if args.dtype is not None and args.dtype != want:
        raise SystemExit(f"--model {args.model} computes in {want} (requested {args.dtype})")
    if args.profile:
        from multidisttorch_amd.obs import trace

        trace.enable()
        if args.metrics_dir is None:
            args.metrics_dir = "metrics"
    ngroups = args.ngroups
    comm_size, rank = setup_ddp()
    processes_groups = setup_ddp_groups(ngroups)
    control_group()  # world collective: create the gloo control plane on every rank
    create_health_groups(ngroups)  # world collective: per-trial gloo health agreement (faults.py)

    T = max(1, args.trials_per_group)
    specs = build_specs(ngroups * T, args.epochs, parse_list(args.lr), parse_list(args.beta), args.seed,
                        epoch_offset=not args.no_epoch_offset, lr_warmups=parse_list(args.lr_warmup, int),
                        lr_decays=parse_list(args.lr_decay, lambda s: s.strip()),
                        lr_decay_steps=parse_list(args.lr_decay_steps, int),
                        lr_min_ratios=parse_list(args.lr_min_ratio), kl_anneals=parse_list(args.kl_anneal, int),
                        **{name: getattr(args, name) for name in objective.NAMES})
    opts = RunOptions(batch_size=args.batch_size, log_interval=args.log_interval,
                      backend=args.backend, use_graphs=not args.no_graphs, graph_steps=args.graph_steps,
                      ckpt_dir=args.ckpt_dir, resume=args.resume, metrics_dir=args.metrics_dir,
                      results=not args.no_results, per_group_results=args.per_group_results,
                      train_samples=args.train_samples, test_samples=args.test_samples,
                      data_dir=args.data_dir,
                      synthetic=False if args.real_data else (True if args.synthetic else None),
                      model=args.model, image_size=args.image_size, bucket_mb=parse_bucket_mb(args.bucket_mb),
                      profile=args.profile, iw_samples=max(0, args.iw_samples), latent_report=args.latent_report,
                      au_threshold=args.au_threshold, binarize=args.binarize,
                      report_objective=objective.reported(specs), sample_report=args.sample_report)
    results = []
    member = False
    for group_id, group in enumerate(processes_groups):
        if dist.get_rank(group) >= 0:
            member = True
            if T == 1:
                results.append(run_trial(specs[group_id], group, opts))
            else:
                results.extend(run_packed_trials(specs[group_id * T:(group_id + 1) * T], group, opts,
                                                 num_trials=ngroups * T))
    if not member:
        idle_rank()

    # aggregate samples/s: every rank's records of its trials, summarized on rank 0 (hpo/aggregate.py)
    gathered = [None] * dist.get_world_size()
    dist.all_gather_object(gathered, [trial_record(r, opts) for r in results], group=control_group())
    if dist.get_rank() == 0:
        summary = summarize(gathered, specs, opts)
        if args.metrics_dir:
            os.makedirs(args.metrics_dir, exist_ok=True)
            with open(os.path.join(args.metrics_dir, "aggregate.json"), "w") as f:
                json.dump(summary, f)
        print("MDT_AGGREGATE " + json.dumps(summary), flush=True)
    # control-plane barrier, then teardown: no rank (an idle leftover one least of all) takes its process
    # groups down while a peer still talks to it -- the gloo teardown race of docs/ROUND6.md, "Teardown"
    global_barrier()
    shutdown()


if __name__ == "__main__":
    main()
