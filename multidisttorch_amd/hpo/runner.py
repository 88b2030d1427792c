"""Per-trial driver: one HPO trial trained by one group of ranks.

Parity map (/root/reference/vae-hpo.py):
  * ``run(group_id, batch_size, epochs, group)`` :122-174  -> ``run_trial``
  * ``train`` :61-92 / ``test`` :95-119                     -> ``_train_epoch`` / ``_test_epoch``
  * stdout formats (``[W:G] Train Epoch: ...``, ``====> Epoch: ...``,
    ``====> Test set loss: ...``, ``"{rank} Done. time: ..."``) are byte
    compatible; ``results-{group_rank}/reconstruction_{e}.png`` and
    ``sample_{e}.png`` keep the reference's layout (SURVEY.md Q7 collision
    included unless ``per_group_results``).
  * the DistributedSampler shard (``rank=group_id, num_replicas=W//group_size``)
    and its fixed epoch order (no ``set_epoch``) are reproduced exactly.

MI355X-first differences: the whole epoch runs as replays of a captured
hipGraph over device-resident data (no DataLoader, no per-step ``.item()``);
the loss history is read once per epoch to print the same log lines; global
barriers run on the gloo control plane so uneven trials never trip the RCCL
watchdog; replicas of a group (size > 1) all-reduce gradients through the
native bucket reducer, overlapped with the tail of the backward pass.
"""

from __future__ import annotations

import math
import os
import struct
import sys
import time
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.distributed as dist

from ..ckpt import checkpoint as ckpt
from ..data.binarize import Binarizer, check_mode
from ..data.datasets import ImageSet
from ..data.sampler import reference_num_replicas, shard_indices
from ..models.trainer_base import LOSS_HIST as LOSS_RING  # per-step loss ring of the trainers
from ..obs.metrics import TrialMetrics
from ..obs import trace
from ..parallel.autotune import autotune_comm
from ..parallel.ddp import broadcast_params, make_arena_reducer
from ..parallel.groups import print0
from ..runtime.bootstrap import bound_device, global_barrier
from ..runtime.faults import (InjectedFault, TrialCorrupted, TrialTimeout, agree_healthy, fault_step, group_timeout_s, guarded,
                              heartbeat_s, maybe_inject, trial_watch)
from ..utils.images import flush_images, save_image_async
from .objective import KNOBS, NAMES
from .schedule import LR_DECAYS, Schedule
from .trial import TrialSpec

__all__ = ["RunOptions", "TrialResult", "run_trial", "run_packed_trials", "idle_rank"]


@dataclass
class RunOptions:
    batch_size: int = 128
    log_interval: int = 10
    model: str = "mlp"
    backend: Optional[str] = None          # hip | torch (default: hip on GPU)
    use_graphs: bool = True
    graph_steps: int = 10
    ckpt_dir: Optional[str] = None
    resume: bool = False
    metrics_dir: Optional[str] = None
    results: bool = True                   # write PNGs like the reference
    per_group_results: bool = False        # opt-in fix for the results-0 collision (Q7)
    eval_each_epoch: bool = True
    quiet_train_log: bool = False
    train_samples: Optional[int] = None    # synthetic dataset size (default 60000)
    test_samples: Optional[int] = None     # (default 10000)
    image_size: int = 28
    data_dir: str = "data"
    synthetic: Optional[bool] = None       # None: IDX files when present, else synthetic; True/False force
    bucket_mb: Optional[object] = None     # None: model default; 0: one bucket; float: MiB cap; "auto": measured
    profile: bool = False                  # roctx ranges + device-synced phase timings in the metrics JSONL
    iw_samples: int = 0                    # K > 0: importance-weighted test log-likelihood after the last epoch
    latent_report: bool = False            # active units + MI / TC / dimension-wise-KL split after the last epoch
    au_threshold: float = 0.01             # a dimension is active when Var_x(mu_d) exceeds this
    binarize: str = "none"                 # none | threshold | static | dynamic (data/binarize.py); one value per run
    report_objective: tuple = ()           # objective.reported(specs): knobs whose values the metrics carry
    sample_report: int = 0                 # N > 0: kernel MMD + 1-NN test of N prior samples against N test rows


@dataclass
class TrialResult:
    group_id: int
    epochs: int
    shard: int
    samples: int
    wall_s: float
    final_train_loss: float = float("nan")
    final_test_loss: float = float("nan")
    failed: bool = False
    error: str = ""
    extra: dict = field(default_factory=dict)


def _results_dir(opts: RunOptions, group_id: int, group_rank: int) -> str:
    if opts.per_group_results:
        return f"results-g{group_id}-{group_rank}"
    return f"results-{group_rank}"


def _schedule_words(s) -> list:
    """A Schedule as six int64 words (flag, W, decay kind, T, A, bits of r) for the resume broadcast."""
    if s is None:
        return [0] * 6
    return [1, s.lr_warmup_steps, LR_DECAYS.index(s.lr_decay), s.lr_decay_steps, s.kl_anneal_steps,
            struct.unpack("<q", struct.pack("<d", s.lr_min_ratio))[0]]


def _schedule_from_words(w):
    if not w[0]:
        return None
    return Schedule(w[1], LR_DECAYS[w[2]], w[3], struct.unpack("<d", struct.pack("<q", w[5]))[0], w[4])


def _total_steps(spec: TrialSpec, opts: RunOptions, n_shard: int) -> int:
    """Optimizer steps of the whole trial: the default cosine horizon."""
    return spec.epochs * -(-n_shard // opts.batch_size)


def _make_trainer(spec: TrialSpec, opts: RunOptions, device, group_rank: int, D: int,
                  total_steps: Optional[int] = None):
    sched = spec.schedule(total_steps)
    sched = sched if sched.active else None
    kw = dict(batch_size=opts.batch_size, device=device, backend=opts.backend, seed=spec.seed, lr=spec.lr,
              kl_beta=spec.beta, rng_stream=group_rank, use_graphs=opts.use_graphs, graph_steps=opts.graph_steps,
              schedule=sched, **spec.objective())
    if opts.model == "mlp":
        from ..models.mlp_trainer import MlpVaeTrainer

        return MlpVaeTrainer(D=D, **kw)
    if opts.model == "conv":
        from ..models.conv_vae import ConvVaeTrainer

        return ConvVaeTrainer(image=opts.image_size, z=32 if opts.image_size == 28 else 64, **kw)
    raise ValueError(f"unknown model {opts.model!r}")


def _load_data(opts: RunOptions, device):
    from ..data.datasets import mnist_like

    train = mnist_like(True, data_dir=opts.data_dir, device=device, size=opts.image_size,
                       synthetic=opts.synthetic, n=opts.train_samples)
    test = mnist_like(False, data_dir=opts.data_dir, device=device, size=opts.image_size,
                      synthetic=opts.synthetic, n=opts.test_samples)
    return train, test


def _check_resumed(prog, spec: TrialSpec, opts: RunOptions):
    """A resumed trial keeps the likelihood (``--binarize``) and the objective (every knob of
    hpo/objective.py) it was trained under; an old checkpoint without the record: none, and 0."""
    asked = [("--binarize", "binarize", "none", opts.binarize)]
    asked += [(k.flag, k.name, 0.0, getattr(spec, k.name)) for k in KNOBS]
    for flag, key, default, want in asked if prog is not None else []:
        had = prog.get(key, default)
        if had != want:
            raise ValueError(f"trial {spec.group_id}: checkpoint {prog['path']} was trained with {flag} "
                             f"{had}, this run asks for {flag} {want}")


def _resume(trainer, spec: TrialSpec, opts: RunOptions, group=None, announce: bool = False):
    """``--resume``: the trial's newest checkpoint restored into ``trainer``, refused if it was
    trained under something else -> (its progress record or None, the epoch to start from)."""
    prog = ckpt.load_latest(opts.ckpt_dir, spec.group_id, trainer) if opts.ckpt_dir and opts.resume else None
    if prog is None:
        return None, 1
    if announce:  # (run_trial: printed once the checkpoint is loaded, refused or not)
        print0(f"resumed trial {spec.group_id} from {prog['path']} (epoch {prog['epoch']})", process_group=group)
    _check_resumed(prog, spec, opts)
    return prog, prog["epoch"] + 1


def _bind_data(trainer, spec: TrialSpec, opts: RunOptions, train, test, idx):
    """Bind the trial's shard ``idx`` of the training rows and do the set-up that precedes the
    timer -> (the shard's Binarizer or None, the test set every pass of the trial reads). With
    ``--binarize`` the trainer reads the binarizer's compact buffer (redrawn in place at the top
    of every epoch, ``_refresh_train``) and every test pass the binarized test rows, drawn here
    once; every trial holds its own buffers."""
    binarizer = None
    if opts.binarize != "none":
        bt = Binarizer(opts.binarize, spec.seed, test.data, torch.arange(len(test), dtype=torch.int32), 1)
        bt.refresh(0)
        test = ImageSet(bt.data, test.shape, test.synthetic, test.name)
        binarizer = Binarizer(opts.binarize, spec.seed, train.data, idx, 0)
        trainer.bind_train_data(binarizer.data, binarizer.index())
    else:
        trainer.bind_train_data(train.data, idx)
    # capture the step graphs and the test-set eval graphs and load the decode kernels now, like the
    # reference's model/DDP construction before its timer starts (vae-hpo.py:159)
    trainer.prepare([opts.batch_size, idx.numel() % opts.batch_size], test.data if opts.eval_each_epoch else None)
    return binarizer, test


def _raw_test_eval(trainer, test, opts: RunOptions, group, metrics, device, tag: str = "") -> dict:
    """Untimed, after a trial's last epoch: one test pass under the raw weights
    of a trial whose scores are under the averaged ones (``test_loss_raw`` in
    the aggregate: what averaging bought). Prints and logs nothing."""
    idx = torch.arange(len(test), dtype=torch.int32, device=test.data.device)
    with trace.range("raw_test_eval"):
        total, _ = trainer.evaluate(test.data, idx, want_first_recon=False)
    return dict(test_loss_raw=total / len(test))


def _refresh_train(binarizer, trainer, epoch: int, opts: RunOptions, device):
    """Top of an epoch, on the stream the epoch is enqueued on: redraw the
    trial's training rows in place (dynamic: every epoch; static / threshold:
    the first one) and tell the trainer. Seconds taken (device-synced under
    ``--profile``), or None without ``--binarize``."""
    if binarizer is None:
        return None
    t = time.perf_counter()
    with trace.range(f"binarize_{epoch}"):
        if binarizer.refresh(epoch):
            trainer.train_data_changed()
        if opts.profile and device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()
    return round(time.perf_counter() - t, 6)


def _steps(trainer, n: int, B: int, events):
    """``train_steps(n)``; with an ``events`` list, in chunks of about 64 steps
    (a whole number of captured graphs) each followed by a recorded event, so
    a waiter can tell a slow epoch that is still completing steps from a stuck
    one."""
    if events is None:
        trainer.train_steps(n, B)
        return
    gs = max(1, int(getattr(trainer, "graph_steps", 1)))
    chunk = gs * max(1, 64 // gs)
    done = 0
    while done < n:
        k = min(chunk, n - done)
        trainer.train_steps(k, B)
        done += k
        ev = torch.cuda.Event()
        ev.record()
        events.append(ev)


def _launch_epoch(trainer, epoch: int, n_shard: int, opts: RunOptions, fault_at: Optional[int] = None,
                  events=None):
    """Enqueue one epoch of steps on the current stream; returns (step counter
    before the epoch, {batch_idx: loss} of log lines whose ring slots were read
    early). No host sync unless the epoch is longer than the loss ring: then
    the ring is read after every LOSS_RING steps, before it wraps (batch sizes
    below 15 on a 60000-sample shard). ``fault_at`` (MDT_FAULT step=) stops
    issuing steps at that optimizer step and raises, mid-epoch. ``events``
    (a list) receives progress events (see ``_steps``)."""
    B = opts.batch_size
    full, tail = n_shard // B, n_shard % B
    nb = full + (1 if tail else 0)
    trainer.set_cursor(0, nb)
    trainer.reset_loss()
    step0 = trainer.step_count
    early = {}
    stop = None if fault_at is None or not step0 <= fault_at < step0 + nb else fault_at - step0
    with trace.range(f"train_epoch_{epoch}"):
        c = 0
        while c < full:
            n = min(full - c, LOSS_RING) if nb > LOSS_RING else full - c
            if stop is not None and c + n > stop:
                _steps(trainer, stop - c, B, events)
                raise InjectedFault(f"injected fault at step {fault_at} (epoch {epoch})")
            _steps(trainer, n, B, events)
            if nb > LOSS_RING:
                hist = trainer.loss_history()
                assert len(hist) == LOSS_RING
                for bi in range(c - c % opts.log_interval, c + n, opts.log_interval):
                    if bi >= c:
                        early[bi] = float(hist[(step0 + bi) % LOSS_RING])
            c += n
        if tail:
            if stop is not None and stop == full:
                raise InjectedFault(f"injected fault at step {fault_at} (epoch {epoch})")
            _steps(trainer, 1, tail, events)
    return step0, early


def _abort(group, device, trainer=None):
    """Give up on the group's data plane: the trainer's xGMI reducer (its
    in-kernel waits see the host-mapped abort word, so the steps still queued
    drain at once instead of one MDT_P2P_TIMEOUT_S each) and the group's RCCL
    communicator (its kernels observe the abort flag and exit)."""
    red = getattr(trainer, "reducer", None)
    if red is not None and hasattr(red, "abort"):
        red.abort()
    try:
        be = group._get_backend(device)
        if hasattr(be, "abort"):
            be.abort()
    except Exception:  # noqa: BLE001 - best effort, we are failing anyway
        pass


def _drain(events, limit_s: float):
    """After an abort: wait (bounded) until the queued steps have left the
    stream, so the process can sync, checkpoint or exit. Seconds taken, or
    None if the stream is still busy after ``limit_s``."""
    t = time.monotonic()
    while events and not events[-1].query():
        if time.monotonic() - t > limit_s:
            return None
        time.sleep(0.001)
    return time.monotonic() - t


def _fail_epoch(trainer, group, device, events, msg):
    _abort(group, device, trainer)
    limit = float(os.getenv("MDT_ABORT_DRAIN_S", "30"))
    d = _drain(events, limit)
    trainer.drain_s = d
    tail = f"stream drained in {d:.2f} s" if d is not None else f"stream still busy after {limit:.0f} s"
    raise TrialTimeout(f"{msg} ({tail})")


def _wait_epoch(trainer, group, device, events, watch=None):
    """Wait for this replica's enqueued epoch (groups > 1 on GPU).

    The bucket collectives run inside replayed graphs, out of sight of
    ProcessGroupNCCL's watchdog: if a peer died mid-epoch they would never
    complete. So: poll the epoch's progress events; meanwhile beat on the
    trial's ``TrialWatch`` and check the peers (a published failure or a
    silent peer ends the wait within ~0.5 s / ``MDT_HEARTBEAT_S``); and if no
    chunk of steps completes for ``MDT_GROUP_TIMEOUT_S`` the epoch is stuck.
    Either way abort the group's data plane (``_abort``: the xGMI reducer's
    waits and the RCCL communicator give up), let the queued steps drain
    (bounded by ``MDT_ABORT_DRAIN_S``) and fail the trial."""
    if device.type != "cuda" or group is None or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    ev = torch.cuda.Event()
    ev.record()
    events.append(ev)
    stall, hb = group_timeout_s(), heartbeat_s()
    now = time.monotonic()
    last_progress, next_beat, done = now, now, 0
    if watch is not None:
        watch.reset()
    while True:
        while done < len(events) and events[done].query():
            done += 1
            last_progress = time.monotonic()
        if done == len(events):
            break
        now = time.monotonic()
        if now - last_progress > stall:
            _fail_epoch(trainer, group, device, events, f"no step of the epoch completed for {stall:.0f} s (peer lost?)")
        if watch is not None and now >= next_beat:
            next_beat = now + 0.5
            try:
                watch.beat()
                msg = watch.check(hb)
            except Exception as e:  # noqa: BLE001 - the store (on world rank 0) is unreachable
                msg = f"control store unreachable: {type(e).__name__}: {e}"
            if msg:
                _fail_epoch(trainer, group, device, events, msg)
        time.sleep(0.0005)
    red = getattr(trainer, "reducer", None)
    if red is not None and hasattr(red, "status") and int(red.status()) != 0:
        raise TrialTimeout(f"p2p all-reduce gave up waiting for a peer (status {int(red.status())})")


def _check_health(trainer):
    """Fail the trial on a kernel-reported corruption (ConvVaeTrainer.health_error)."""
    fn = getattr(trainer, "health_error", None)
    msg = fn() if fn is not None else None
    if msg:
        raise TrialCorrupted(msg)


def _train_epoch(trainer, epoch: int, n_shard: int, n_dataset: int, opts: RunOptions, group,
                 step0: Optional[int] = None, tag: str = "", fault_at: Optional[int] = None, watch=None) -> float:
    B = opts.batch_size
    full, tail = n_shard // B, n_shard % B
    nb = full + (1 if tail else 0)
    early = {}
    if step0 is None:
        device = getattr(trainer, "device", torch.device("cpu"))
        multi = device.type == "cuda" and group is not None and dist.is_initialized() and \
            dist.get_world_size(group) > 1
        events = [] if multi else None
        step0, early = _launch_epoch(trainer, epoch, n_shard, opts, fault_at, events)
        _wait_epoch(trainer, group, device, events, watch)
    elif nb > LOSS_RING:
        raise ValueError(f"{nb} batches per epoch exceed the {LOSS_RING}-entry loss ring of a packed trial; "
                         f"use a larger --batch-size or --trials-per-group 1")
    _check_health(trainer)
    hist = trainer.loss_history()
    st = trainer.read_state()
    if not opts.quiet_train_log:
        for batch_idx in range(0, nb, opts.log_interval):
            bsz = B if batch_idx < full else tail
            loss_b = early.get(batch_idx)
            if loss_b is None:
                loss_b = float(hist[(step0 + batch_idx) % len(hist)])
            print0(tag + "Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}".format(
                epoch, batch_idx * bsz, n_dataset, 100.0 * batch_idx / nb, loss_b / bsz), process_group=group)
    # The reference divides by the FULL dataset size, not the shard (Q6).
    print0(tag + "====> Epoch: {} Average loss: {:.4f}".format(epoch, st["epoch_loss"] / n_dataset),
           process_group=group)
    return st["epoch_loss"]


def _test_epoch(trainer, epoch: int, test, opts: RunOptions, group, rdir: Optional[str], shape,
                tag: str = "") -> float:
    idx = torch.arange(len(test), dtype=torch.int32, device=test.data.device)
    # averaged_weights(): every score of a trial with --ema-decay is under its weight average (a no-op without)
    with trace.range(f"test_epoch_{epoch}"), trainer.averaged_weights():
        total, first = trainer.evaluate(test.data, idx, want_first_recon=rdir is not None)
    if rdir is not None and first is not None:
        m = first.shape[0]
        n = min(m, 8)
        data = test.data[:n].view(n, *shape).float().cpu()
        comparison = torch.cat([data, first[:n].view(n, *shape).float().cpu()])
        os.makedirs(rdir, exist_ok=True)
        save_image_async(comparison, f"{rdir}/reconstruction_" + str(epoch) + ".png", nrow=n)
    test_loss = total / len(test)
    print0(tag + "====> Test set loss: {:.4f}".format(test_loss), process_group=group)
    return test_loss


def _iw_eval(trainer, test, opts: RunOptions, group, metrics, device, tag: str = "") -> dict:
    """One importance-weighted pass over the test set after a trial's last
    epoch (``--iw-samples K``): the K-sample bound on -log p(x) and the
    K-sample negative ELBO at beta = 1, per-image means. Unlike the test loss
    they do not depend on the trial's beta, so trials of a beta sweep compare.
    Runs after the trial's wall time was taken: samples/s is unaffected."""
    K = int(opts.iw_samples)
    t = time.perf_counter()
    idx = torch.arange(len(test), dtype=torch.int32, device=test.data.device)
    with trace.range("iw_eval"), trainer.averaged_weights():
        r = trainer.evaluate_iw(test.data, idx, K)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
    out = dict(iw_nll=r["nll"] / len(test), iw_neg_elbo=r["neg_elbo"] / len(test), iw_samples=K,
               iw_s=round(time.perf_counter() - t, 6))
    print0(tag + "====> Test set IW-{} NLL: {:.4f} ELBO-{}: {:.4f}".format(K, out["iw_nll"], K, out["iw_neg_elbo"]),
           process_group=group)
    metrics.log(event="iw_eval", **out)
    return out


def _latent_eval(trainer, test, opts: RunOptions, group, metrics, device, tag: str = "") -> dict:
    """One latent report pass over the test set after a trial's last epoch
    (``--latent-report``, models/latent.py): the analytic KL per dimension, the
    active units and the split of the KL term into mutual information, total
    correlation and dimension-wise KL -- why the trial scored as it did. Like
    the IW pass it runs after the trial's wall time was taken."""
    t = time.perf_counter()
    idx = torch.arange(len(test), dtype=torch.int32, device=test.data.device)
    with trace.range("latent_eval"), trainer.averaged_weights():
        r = trainer.evaluate_latent(test.data, idx, au_threshold=opts.au_threshold)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
    r = {k: ([round(float(x), 6) for x in v.tolist()] if torch.is_tensor(v) else v) for k, v in r.items()}
    r["latent_s"] = round(time.perf_counter() - t, 6)
    print0(tag + "====> Test set latent: KL {:.4f} active {}/{} MI {:.4f} TC {:.4f} DWKL {:.4f}".format(
        r["kl"], r["active_units"], len(r["kl_per_dim"]), r["mi"], r["tc"], r["dwkl"]), process_group=group)
    fb = float(trainer.hp.get("free_bits", 0.0))
    if fb > 0:
        # dimensions the floor holds up: their test-set mean KL (the true one) is below it
        r["free_bits"] = fb
        r["below_floor"] = sum(1 for v in r["kl_per_dim"] if v < fb)
    metrics.log(event="latent_eval", **r)
    return dict(latent=r)


def _check_sample_rows(opts: RunOptions, test):
    """At run start: ``--sample-report N`` needs N test rows."""
    if opts.sample_report > len(test):
        raise ValueError(f"--sample-report {opts.sample_report} exceeds the test set's {len(test)} rows")


def _sample_eval(trainer, test, opts: RunOptions, group, metrics, device, tag: str = "") -> dict:
    """One sample report pass after a trial's last epoch (``--sample-report N``,
    models/sample_report.py): the kernel MMD and the 1-NN two-sample test between
    N decoded prior samples and the first N test rows -- what the decoder makes of
    the prior, which neither the test loss nor the IW bound looks at. Like its
    siblings it runs after the trial's wall time was taken."""
    n = int(opts.sample_report)
    _check_sample_rows(opts, test)
    t = time.perf_counter()
    idx = torch.arange(n, dtype=torch.int32, device=test.data.device)
    with trace.range("sample_eval"), trainer.averaged_weights():
        r = trainer.evaluate_samples(test.data, idx, n)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
    r["sample_s"] = round(time.perf_counter() - t, 6)
    print0(tag + "====> Test set samples: MMD2 {:.6f} 1-NN acc {:.4f} (real {:.4f} gen {:.4f})".format(
        r["mmd2"], r["nn_acc"], r["nn_acc_real"], r["nn_acc_fake"]), process_group=group)
    metrics.log(event="sample_eval", **r)
    return dict(sample_report=r)


# after a trial's last epoch and its wall time, in this order: (label, enabled(spec, opts), pass -> part of extra)
_AFTER_TRIAL = (
    ("IW pass", lambda spec, opts: opts.iw_samples > 0, _iw_eval),
    ("latent pass", lambda spec, opts: opts.latent_report, _latent_eval),
    ("raw-weight test pass", lambda spec, opts: spec.ema_decay > 0, _raw_test_eval),
    ("sample pass", lambda spec, opts: opts.sample_report > 0, _sample_eval),
)


def _after_trial(trainer, spec: TrialSpec, test, opts: RunOptions, group, metrics, device, failure: dict,
                 world_rank: int, tag: str = "") -> dict:
    """-> ``extra`` of a trial that has not failed; a pass that raises fails it and ends the list."""
    extra = {}
    for label, enabled, run in _AFTER_TRIAL:
        if enabled(spec, opts) and not failure:
            with guarded(f"trial {spec.group_id} {label} (world rank {world_rank})", None,
                         lambda e: failure.setdefault("error", f"{type(e).__name__}: {e}")):
                extra.update(run(trainer, test, opts, group, metrics, device, tag=tag))
    return extra


def run_trial(spec: TrialSpec, group, opts: RunOptions, data=None, num_trials: Optional[int] = None) -> TrialResult:
    """Train one trial on the ranks of ``group`` (this rank is a member)."""
    check_mode(opts.binarize)
    world_rank = dist.get_rank() if dist.is_initialized() else 0
    world_size = dist.get_world_size() if dist.is_initialized() else 1
    grank = dist.get_rank(group) if dist.is_initialized() else 0
    gsize = dist.get_world_size(group) if dist.is_initialized() else 1
    # sampler replicas exactly as the reference (vae-hpo.py:146): W // group size,
    # which differs from the trial count K when W % K != 0 (leftover idle ranks)
    n_rep = reference_num_replicas(world_size, gsize)
    device = bound_device()

    train, test = data if data is not None else _load_data(opts, device)
    _check_sample_rows(opts, test)
    if grank == 0:  # stderr: stdout stays byte-compatible with the reference
        print(f"[mdt] trial {spec.group_id}: train data {train.name} ({'synthetic' if train.synthetic else 'IDX'}, "
              f"{len(train)} x {tuple(train.shape)})", file=sys.stderr, flush=True)
    D = int(train.data.shape[1])
    idx = shard_indices(len(train), n_rep, spec.group_id)
    n_shard = idx.numel()
    total_steps = _total_steps(spec, opts, n_shard)
    trainer = _make_trainer(spec, opts, device, grank, D, total_steps)
    if gsize > 1:
        # DDP's _sync_module_states: replicas start from group rank 0's weights
        broadcast_params([trainer.params], group)
        trainer.refresh_weights()
        trainer.reset_average()  # the average starts as the weights every replica now holds
        if opts.bucket_mb == "auto":
            key = f"{opts.model}-{opts.image_size}-b{opts.batch_size}-n{trainer.numel}-s{gsize}"
            bounds, kind, timings = autotune_comm(
                lambda: _make_trainer(spec, opts, device, grank, D, total_steps), group, train.data, idx, key=key)
            print0(f"bucket autotune (group of {gsize}): {timings} -> {kind or 'default'} {bounds}",
                   process_group=group)
        else:
            bounds, kind = trainer.bucket_bounds(opts.bucket_mb), None
        trainer.attach_reducer(make_arena_reducer(group, trainer.grads, bounds, kind=kind,
                                                  comm_jobs=getattr(trainer, "comm_jobs", False)))
    prog, start_epoch = None, 1
    if opts.ckpt_dir and opts.resume:
        # only group rank 0 writes checkpoints, so only it reads one; the replicas receive weights, Adam
        # moments, the step counter and the epoch to resume from (no shared filesystem needed). Rank 0's
        # load outcome goes first, so a load error (arch mismatch, corrupt file, another objective) raises
        # on every member together instead of stranding the replicas in the parameter broadcast.
        err = None
        if grank == 0:
            try:
                prog, start_epoch = _resume(trainer, spec, opts, group, announce=True)
            except Exception as e:  # noqa: BLE001 - re-raised below on every member
                err = e
        if gsize > 1:
            # + the schedule rank 0's checkpoint restored (it wins over the command line on every member)
            meta = torch.tensor([0 if err is None else 1, start_epoch, trainer.step_count] +
                                _schedule_words(trainer.schedule if prog is not None else None), dtype=torch.int64,
                                device=device if dist.get_backend(group) == "nccl" else "cpu")
            broadcast_params([meta], group)
            if int(meta[0].item()) != 0:
                if err is not None:
                    raise err
                raise RuntimeError(f"trial {spec.group_id}: group rank 0 could not load its checkpoint; "
                                   f"stopping every member")
            broadcast_params([trainer.params, trainer.exp_avg, trainer.exp_avg_sq] +
                             ([trainer.ema] if trainer.ema_on else []), group)
            start_epoch = int(meta[1].item())
            sched = _schedule_from_words([int(v) for v in meta[3:].tolist()])
            if sched is not None:
                trainer.set_schedule(sched)
            trainer.set_step(int(meta[2].item()))
            trainer.refresh_weights()
        elif err is not None:
            raise err
    metrics = TrialMetrics(opts.metrics_dir, spec.group_id, enabled=(grank == 0))
    binarizer, test = _bind_data(trainer, spec, opts, train, test, idx)

    # Parity with the reference's download barrier (vae-hpo.py:133-144).
    global_barrier()
    rdir = _results_dir(opts, spec.group_id, grank) if opts.results else None
    shape = (1, opts.image_size, opts.image_size)
    gen = torch.Generator(device="cpu").manual_seed(spec.seed * 7919 + 17)

    t0 = time.time()
    train_loss = test_loss = float("nan")
    failure = {}
    epochs_done = 0

    watch = trial_watch(spec.group_id) if gsize > 1 else None

    def _fail(e):
        failure["error"] = f"{type(e).__name__}: {e}"
        metrics.log(event="trial_failed", error=failure["error"])
        if watch is not None:  # peers waiting on their epoch see it within ~0.5 s
            watch.fail(failure["error"])

    fault_at = fault_step(trial=spec.group_id, rank=world_rank)
    checked_in = False  # this member's "not ok" has been delivered to the group
    with guarded(f"trial {spec.group_id} (world rank {world_rank})", group, _fail):
        for epoch in range(start_epoch, spec.epochs + 1):
            # group members agree on health before every epoch (see faults.py)
            if not agree_healthy(spec.group_id, True):
                checked_in = True
                raise RuntimeError("a replica of this trial failed; stopping the trial on every member")
            maybe_inject(trial=spec.group_id, epoch=epoch, rank=world_rank)
            train_loss, test_loss = _run_epoch(trainer, epoch, n_shard, train, test, opts, group, rdir, shape,
                                               gen, device, spec, grank, metrics, fault_at=fault_at, watch=watch,
                                               binarizer=binarizer)
            epochs_done += 1
        if not agree_healthy(spec.group_id, True):
            checked_in = True
            raise RuntimeError("a replica of this trial failed in its last epoch")
    if failure and not checked_in:
        agree_healthy(spec.group_id, False)

    flush_images()
    global_barrier()  # parity: vae-hpo.py:172 (waits for the slowest trial)
    t1 = time.time()
    print(world_rank, "Done. time: %f" % (t1 - t0), flush=True)
    extra = _after_trial(trainer, spec, test, opts, group, metrics, device, failure, world_rank)
    return TrialResult(spec.group_id, epochs_done, n_shard, epochs_done * n_shard, t1 - t0,
                       train_loss / len(train), test_loss, failed=bool(failure), error=failure.get("error", ""),
                       extra=extra)


def _objective_metrics(st, spec: TrialSpec, opts: RunOptions, n_shard: int) -> dict:
    """The knob part of an epoch's record: the value in force at the epoch's last step where the
    kernels record one (``st = trainer.read_state()``), the value the trial was given otherwise."""
    out = {}
    for name in (n for n in NAMES if n in opts.report_objective):
        if name == "tc_weight":  # + the epoch's sum of tc_batch (unweighted, models/tc.py) over the rows trained
            out["train_tc"] = st["epoch_tc"] / max(n_shard, 1)
        out[name] = st[name] if name in st else getattr(spec, name)
    return out


def _run_epoch(trainer, epoch, n_shard, train, test, opts, group, rdir, shape, gen, device, spec, grank, metrics,
               step0=None, t_train=None, tag="", fault_at=None, watch=None, binarizer=None, binarize_s=None):
    te = time.perf_counter()
    if step0 is None:  # (packed trials redraw where they enqueue their epoch)
        binarize_s = _refresh_train(binarizer, trainer, epoch, opts, device)
    train_loss = _train_epoch(trainer, epoch, n_shard, len(train), opts, group, step0=step0, tag=tag,
                              fault_at=fault_at, watch=watch)
    if t_train is None:
        t_train = time.perf_counter() - te
    phases = {} if binarize_s is None or not opts.profile else {"binarize_s": binarize_s}

    def _mark(name, t):
        if opts.profile and device.type == "cuda":
            torch.cuda.synchronize(device)
        phases[name] = round(time.perf_counter() - t, 6)
        return time.perf_counter()

    t = time.perf_counter()
    test_loss = float("nan")
    if opts.eval_each_epoch:
        test_loss = _test_epoch(trainer, epoch, test, opts, group, rdir, shape, tag=tag)
    t = _mark("eval_s", t)
    if rdir is not None:
        with torch.no_grad(), trace.range(f"sample_{epoch}"), trainer.averaged_weights():
            sample = torch.randn(64, trainer.Z, generator=gen).to(device)
            sample = trainer.decode(sample).cpu()
            os.makedirs(rdir, exist_ok=True)
            save_image_async(sample.view(64, *shape), f"{rdir}/sample_" + str(epoch) + ".png")
    t = _mark("sample_s", t)
    if opts.ckpt_dir and grank == 0:
        with trace.range(f"ckpt_{epoch}"):
            ckpt.save_trial(opts.ckpt_dir, trainer, spec, epoch, binarize=opts.binarize)
    _mark("ckpt_s", t)
    # lr / kl_beta: the effective values of the epoch's last step as the kernels
    # recorded them (= lr_base / beta when the trial has no schedule)
    st = trainer.read_state()
    metrics.log(epoch=epoch, train_loss_sum=train_loss, train_loss=train_loss / len(train),
                test_loss=test_loss, epoch_train_s=t_train, samples=n_shard,
                train_samples_per_s=n_shard / max(t_train, 1e-9), lr=st["lr"], kl_beta=st["kl_beta"],
                lr_base=spec.lr, beta=spec.beta, **_objective_metrics(st, spec, opts, n_shard), **phases)
    return train_loss, test_loss


def run_packed_trials(specs, group, opts: RunOptions, data=None, num_trials: Optional[int] = None):
    """Train several trials concurrently on this rank's GPU (trial packing).

    MI355X-first extension (no reference counterpart): one small VAE step
    fills only part of the 256 CUs, so T trials of a size-1 group each get a
    HIP stream and their captured step graphs are replayed concurrently
    (measured 1.6-1.8x aggregate throughput at T = 2, profiles/r1_packing).
    Per epoch: every live trial's steps are enqueued on its stream, one
    device sync, then per-trial logging / eval / samples / checkpoints exactly
    as ``run_trial`` does (lines carry a ``(trial t)`` tag). Each trial is
    failure-isolated; uneven epoch counts are handled per trial.
    """
    world_rank = dist.get_rank() if dist.is_initialized() else 0
    world_size = dist.get_world_size() if dist.is_initialized() else 1
    gsize = dist.get_world_size(group) if dist.is_initialized() else 1
    check_mode(opts.binarize)
    if gsize != 1:
        raise ValueError("trial packing runs independent trials: it needs groups of one rank")
    total = num_trials if num_trials is not None else world_size * len(specs)
    device = bound_device()
    train, test = data if data is not None else _load_data(opts, device)
    _check_sample_rows(opts, test)
    D = int(train.data.shape[1])
    shape = (1, opts.image_size, opts.image_size)
    tr = []
    for spec in specs:
        idx = shard_indices(len(train), total, spec.group_id)  # packing extension: one shard per trial
        trainer = _make_trainer(spec, opts, device, 0, D, _total_steps(spec, opts, idx.numel()))
        if len(specs) > 1 and hasattr(trainer, "f28_pair"):
            # packed trials fill the chip already; the one-workgroup-per-sample
            # step keeps their numerics independent of how the trials interleave
            trainer.f28_pair = False
        _, start = _resume(trainer, spec, opts)
        binarizer, ttest = _bind_data(trainer, spec, opts, train, test, idx)  # --binarize: a buffer pair per trial
        rdir = (f"results-t{spec.group_id}-0" if opts.results else None)
        tr.append(dict(spec=spec, trainer=trainer, start=start, n_shard=idx.numel(), rdir=rdir,
                       stream=torch.cuda.Stream(device) if device.type == "cuda" else None,
                       metrics=TrialMetrics(opts.metrics_dir, spec.group_id, enabled=True),
                       gen=torch.Generator(device="cpu").manual_seed(spec.seed * 7919 + 17),
                       done=0, train_loss=float("nan"), test_loss=float("nan"), failure={},
                       binarizer=binarizer, test=ttest, binarize_s=None))
    for t in tr:  # a packed epoch is enqueued whole: its losses must fit the ring (checked before any launch)
        nb = -(-t["n_shard"] // opts.batch_size)
        if nb > LOSS_RING:
            raise ValueError(f"{nb} batches per epoch exceed the {LOSS_RING}-entry loss ring of a packed trial; "
                             f"use a larger --batch-size or --trials-per-group 1")
    global_barrier()
    t0 = time.time()
    last = max(t["spec"].epochs for t in tr)
    for epoch in range(1, last + 1):
        live = [t for t in tr if t["start"] <= epoch <= t["spec"].epochs and not t["failure"]]
        te = time.perf_counter()
        for t in live:  # enqueue every trial's epoch on its own stream
            with guarded(f"trial {t['spec'].group_id} (world rank {world_rank})", None,
                         lambda e, t=t: t["failure"].setdefault("error", f"{type(e).__name__}: {e}")):
                maybe_inject(trial=t["spec"].group_id, epoch=epoch, rank=world_rank)
                if t["stream"] is not None:
                    with torch.cuda.stream(t["stream"]):
                        t["binarize_s"] = _refresh_train(t["binarizer"], t["trainer"], epoch, opts, device)
                        t["step0"], _ = _launch_epoch(t["trainer"], epoch, t["n_shard"], opts)
                else:
                    t["binarize_s"] = _refresh_train(t["binarizer"], t["trainer"], epoch, opts, device)
                    t["step0"], _ = _launch_epoch(t["trainer"], epoch, t["n_shard"], opts)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        t_train = time.perf_counter() - te
        for t in live:
            if t["failure"]:
                continue
            spec = t["spec"]
            with guarded(f"trial {spec.group_id} (world rank {world_rank})", None,
                         lambda e, t=t: t["failure"].setdefault("error", f"{type(e).__name__}: {e}")):
                t["train_loss"], t["test_loss"] = _run_epoch(
                    t["trainer"], epoch, t["n_shard"], train, t["test"], opts, group, t["rdir"], shape, t["gen"],
                    device, spec, 0, t["metrics"], step0=t["step0"], t_train=t_train,
                    tag=f"(trial {spec.group_id}) ", binarize_s=t["binarize_s"])
                t["done"] += 1
    flush_images()
    global_barrier()
    t1 = time.time()
    print(world_rank, "Done. time: %f" % (t1 - t0), flush=True)
    for t in tr:
        t["extra"] = _after_trial(t["trainer"], t["spec"], t["test"], opts, group, t["metrics"], device, t["failure"],
                                  world_rank, tag=f"(trial {t['spec'].group_id}) ")
    return [TrialResult(t["spec"].group_id, t["done"], t["n_shard"], t["done"] * t["n_shard"], t1 - t0,
                        t["train_loss"] / len(train), t["test_loss"], failed=bool(t["failure"]),
                        error=t["failure"].get("error", ""), extra=t["extra"]) for t in tr]


def idle_rank():
    """Leftover ranks (W % K) own no trial but join both global barriers, so the
    members never block on them (fixes the reference's crash)."""
    global_barrier()
    t0 = time.time()
    global_barrier()
    return time.time() - t0
