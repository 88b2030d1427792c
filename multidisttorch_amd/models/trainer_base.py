"""What ``MlpVaeTrainer`` and ``ConvVaeTrainer`` share: the driver-facing API
of one HPO trial over flat fp32 arenas (``params`` / ``grads`` / ``exp_avg`` /
``exp_avg_sq`` with a ``layout`` of ``(name, offset, shape)``).

* ``backend="hip"``: the trial's step counter, cursor, loss ring and
  hyper-parameters live on the device in ``self.state`` (``_C.TrialState``,
  csrc/runtime/trial_state.h), so a step (or S steps) is captured in one
  hipGraph and replayed; the loss is read at log points only.
* ``backend="torch"``: the same bookkeeping in host dicts (``_st`` /
  ``_st_eval``) and numpy rings.

A subclass sets ``B``, ``Z``, ``layout``, ``numel``, the arenas and (hip)
``self.state``, then calls ``_push_hparams()``; it provides ``_step_hip(M)``,
``_step_torch(M)``, ``_eval_batch_torch`` and the hip hooks of the
``eval_graphs`` mixins.
"""

from __future__ import annotations

import contextlib
import functools
import os
from typing import Dict, Optional

import numpy as np
import torch

from ..hpo import objective
from ..hpo.schedule import Schedule
from ..ops import native
from ..ops.philox import reparam_eps
from .eval_graphs import GraphedEval, GraphedIwEval, GraphedLatentEval, SampleEval, capture_replayable
from .mlp_vae import views

__all__ = ["VaeTrainerBase", "LOSS_HIST", "EVAL_STREAM", "check_free_bits", "check_ema_decay", "ema_omd"]

EVAL_STREAM = 1 << 30
LOSS_HIST = 4096  # per-step loss ring of a trial state (kLossHist, csrc/kernels/vae_mlp.h)


check_free_bits = functools.partial(objective.check, "free_bits")  # the floor in nats per latent element
check_ema_decay = functools.partial(objective.check, "ema_decay")  # the decay of the weight average, 0 = off


def ema_omd(decay: float, t: int) -> float:
    """1 - d_t of optimizer step t (1-based) as the float32 every element is
    multiplied by, d_t = min(decay, (1 + t) / (10 + t)) in double
    (csrc/kernels/ema.h::ema_omd; docs/KERNELS.md, "Weight averaging")."""
    return float(np.float32(1.0 - min(float(decay), (1.0 + t) / (10.0 + t))))


class VaeTrainerBase(GraphedEval, GraphedIwEval, GraphedLatentEval, SampleEval):
    def __init__(self, batch_size: int, device, backend: Optional[str], seed: int, rng_stream: int, lr: float,
                 kl_beta: float, betas, eps: float, weight_decay: float, decoupled_wd: bool, use_graphs: bool,
                 graph_steps: int, schedule: Optional[Schedule], knobs: Optional[dict] = None):
        self.B = batch_size
        # lr warm-up / cosine decay and KL annealing (hpo/schedule.py); None = off.
        # On the hip backend the kernels evaluate it from the device step counter.
        self.schedule = schedule
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        if backend is None:
            backend = "hip" if self.device.type == "cuda" else "torch"
        if backend == "hip" and self.device.type != "cuda":
            raise ValueError("hip backend needs a GPU device")
        self.backend = backend
        self.seed, self.rng_stream = int(seed), int(rng_stream)
        self.hp = dict(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay,
                       kl_beta=kl_beta, grad_scale=1.0,
                       **{n: objective.check(n, (knobs or {}).get(n, 0.0)) for n in objective.NAMES})
        # the structural knobs (hpo/objective.py) the trainer is built with: its step launches their kernels (a
        # value of 0 later only zeroes their effect); one built without cannot be given a value later
        self._built = {n for n in objective.NAMES if objective.BY_NAME[n].structural and self.hp[n] > 0}
        # total-correlation penalty (models/tc.py): the penalty's kernels in every training step
        self.tc_on = "tc_weight" in self._built
        # weight averaging (docs/KERNELS.md): ``self.ema``, a second arena, updated by every step's last launch
        self.ema_on = "ema_decay" in self._built
        self.ema = None
        self._averaged = False  # inside ``averaged_weights()``: params and ema are exchanged
        self.decoupled_wd = decoupled_wd
        self.use_graphs = use_graphs and backend == "hip"
        self.graph_steps = max(1, int(graph_steps))
        self._graphs: Dict[tuple, "torch.cuda.CUDAGraph"] = {}
        self.reducer = None
        # DDP structure (MDT_DDP_OVERLAP): True = the first-ready bucket goes
        # out while the rest of the backward runs; False = the whole backward,
        # then every bucket inline; None (auto) = overlap only when that
        # bucket's transfer over one xGMI link outweighs the measured cost of
        # splitting the backward (parallel/ddp.py::overlap_pays)
        ov = os.getenv("MDT_DDP_OVERLAP", "auto")
        self.ddp_overlap = None if ov == "auto" else ov != "0"
        self._data = None
        self.state = None  # hip: the subclass's _C.TrialState
        if backend == "hip":
            assert native.require().kLossHist == LOSS_HIST, "C++/Python loss ring lengths disagree"
        else:
            self._st = dict(step=0, cursor=0, nbatches=0, epoch_loss=0.0, epoch_count=0.0, epoch_tc=0.0)
            self._st_eval = dict(self._st)
            self._hist = np.zeros(LOSS_HIST, np.float32)
            self._hist_eval = np.zeros(LOSS_HIST, np.float32)

    # ------------------------------------------------------------------ params
    def named_parameters(self) -> Dict[str, torch.Tensor]:
        return views(self.params, self.layout)

    def named_grads(self) -> Dict[str, torch.Tensor]:
        return views(self.grads, self.layout)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Model weights under the reference's parameter names (cpu copies)."""
        return {k: v.detach().cpu().clone() for k, v in self.named_parameters().items()}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        self._not_averaged("load_state_dict")
        for k, t in self.named_parameters().items():
            t.copy_(sd[k].to(t.device, torch.float32))
        self.refresh_weights()
        self.reset_average()

    def refresh_weights(self):
        """Re-derive the compute copies of the weights after ``params`` changed
        outside a step (replica broadcast, checkpoint load). Nothing to do
        where the params are the compute weights."""

    def optimizer_state(self) -> dict:
        self._not_averaged("optimizer_state")
        st = {"step": self.step_count, "exp_avg": self.exp_avg.detach().cpu().clone(),
              "exp_avg_sq": self.exp_avg_sq.detach().cpu().clone()}
        if self.ema_on:
            st["ema"] = self.ema.detach().cpu().clone()
        return st

    @torch.no_grad()
    def load_optimizer_state(self, st: dict):
        """Adam moments, the step and, when ``ema_on``, the weight average; a
        state without one (a checkpoint of a run without averaging) sets the
        average to the parameters as they are now."""
        self._not_averaged("load_optimizer_state")
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        self.set_step(int(st["step"]))
        if self.ema_on:
            if st.get("ema") is not None:
                self.ema.copy_(st["ema"])
            else:
                self.reset_average()

    # ------------------------------------------------------------------ weight averaging
    def _ema_alloc(self):
        """End of a subclass's construction (arenas exist, params initialised):
        the average starts as the parameters."""
        if self.ema_on:
            self.ema = self.params.detach().clone()

    @torch.no_grad()
    def reset_average(self):
        """e = p: the parameters were set from outside a step (construction,
        ``load_state_dict``, the replica broadcast)."""
        if self.ema_on and self.ema is not None:
            self._not_averaged("reset_average")
            self.ema.copy_(self.params)

    def _not_averaged(self, what: str):
        if self._averaged:
            raise RuntimeError(f"{what} inside averaged_weights(): the parameter arena holds the average")

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The averaged weights under the reference's parameter names (cpu
        copies); the raw weights of a trainer without averaging."""
        self._not_averaged("ema_state_dict")
        src = self.ema if self.ema_on else self.params
        return {k: v.detach().cpu().clone() for k, v in views(src, self.layout).items()}

    @torch.no_grad()
    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]):
        if not self.ema_on:
            raise ValueError("load_ema_state_dict needs a trainer built with ema_decay > 0")
        self._not_averaged("load_ema_state_dict")
        for k, t in views(self.ema, self.layout).items():
            t.copy_(sd[k].to(t.device, torch.float32))

    def _ema_step_hip(self):
        """Last launch of every hip training step of an ``ema_on`` trainer
        (csrc/kernels/ema.hip): the step's optimizer tail has advanced the step
        and written the parameters."""
        if self.ema_on:
            native.require().ema_update(self.ema, self.params, self.numel, state=self.state.train_state,
                                        hparams=self.state.hparams)

    @torch.no_grad()
    def _ema_step_torch(self, t: int):
        """torch backends: the same rule after Adam of optimizer step t, one
        multiply-add per element on the float32 difference ``p - e``. The
        product is exact in float64, so the sum is rounded there and once more
        to float32; ``e == p`` stays a bitwise fixed point."""
        if self.ema_on:
            omd = ema_omd(self.hp["ema_decay"], t)
            d = (self.params - self.ema).double()
            self.ema.copy_((self.ema.double() + omd * d).float())

    def _swap_average(self):
        if self.backend == "hip":
            native.require().arena_swap(self.params, self.ema, self.numel)
        else:
            tmp = self.params.clone()
            self.params.copy_(self.ema)
            self.ema.copy_(tmp)
        self._refresh_swapped()

    def _refresh_swapped(self):
        """The compute copies after ``params`` and ``ema`` were exchanged."""
        self.refresh_weights()

    @contextlib.contextmanager
    def averaged_weights(self):
        """Every compute copy of the weights is the averaged one inside the
        block and the raw one again after it: the two arenas are exchanged in
        place (``arena_swap``) and the derived copies refreshed, so no pointer
        changes and captured eval / IW / latent graphs stay valid. No-op
        without ``ema_on``. Nesting raises, and so does training inside."""
        if self._averaged:
            raise RuntimeError("averaged_weights() does not nest")
        if not self.ema_on:
            yield self
            return
        self._swap_average()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            self._swap_average()

    # ------------------------------------------------------------------ hparams
    def set_hparams(self, **kw):
        for k, v in kw.items():
            if k not in self.hp:
                raise KeyError(k)
            self.hp[k] = objective.check(k, v, self._built) if k in objective.BY_NAME else float(v)
        self._push_hparams()

    def set_schedule(self, schedule: Optional[Schedule]):
        """Replace the schedule (None = off). It continues from the current
        step; captured step graphs stay valid (the parameters are device-resident)."""
        self.schedule = schedule
        self._push_hparams()

    def _push_hparams(self):
        if self.state is not None:
            h = self.hp
            self.state.set_hparams(h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["kl_beta"],
                                   h["grad_scale"], self.seed, self.decoupled_wd,
                                   **(self.schedule or Schedule()).native_args(),
                                   **{n: h[n] for n in objective.NAMES})

    def _effective(self, t: int):
        """(lr_t, beta_t) of optimizer step t on the torch backend, as doubles:
        lr * f_lr(t) and kl_beta * f_kl(t), the products the device forms."""
        s, h = self.schedule, self.hp
        if s is None:
            return h["lr"], h["kl_beta"]
        return h["lr"] * s.lr_factor(t), h["kl_beta"] * s.kl_factor(t)

    def _tc_effective(self, t: int) -> float:
        """tc_t of optimizer step t on the torch backend: the float32 of
        tc_weight * f_kl(t), as the device forms it (sched_store)."""
        s, w = self.schedule, float(np.float32(self.hp["tc_weight"]))
        return float(np.float32(w * (s.kl_factor(t) if s is not None else 1.0)))

    def _tc_alloc(self):
        """hip backend: the penalty's workspace for any M <= B, its value and
        the buffer of its share of d[mu|lv] (csrc/kernels/vae_tc.hip)."""
        C, dev = native.require(), self.device
        n = max(C.tc_ws_numel(m, self.Z) for m in range(1, self.B + 1))
        self.tc_ws = torch.zeros(n, dtype=torch.float32, device=dev)
        self.tc_value = torch.zeros(1, dtype=torch.float64, device=dev)
        self.tc_add = torch.zeros(self.B, 2 * self.Z, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ state
    @property
    def step_count(self) -> int:
        if self.state is not None:
            return int(self.state.read_state(False)[0])
        return self._st["step"]

    def set_step(self, step: int):
        if self.state is not None:
            self.state.set_step(False, int(step))
        else:
            self._st["step"] = int(step)

    def set_cursor(self, cursor: int, nbatches: int, eval: bool = False):
        if self.state is not None:
            self.state.set_cursor(eval, int(cursor), int(nbatches))
        else:
            st = self._st_eval if eval else self._st
            st["cursor"], st["nbatches"] = int(cursor), int(nbatches)

    def reset_loss(self, eval: bool = False):
        if self.state is not None:
            self.state.reset_loss(eval)
        else:
            st = self._st_eval if eval else self._st
            st["epoch_loss"], st["epoch_count"], st["epoch_tc"] = 0.0, 0.0, 0.0

    def read_state(self, eval: bool = False) -> dict:
        if self.state is not None:
            s, t = self.state.read_state(eval), self.state.read_tc(eval)
            return dict(step=int(s[0]), cursor=int(s[1]), nbatches=int(s[2]), epoch_loss=s[3],
                        epoch_count=s[4], lr=s[5], kl_beta=s[6], free_bits=s[7], tc_weight=t[0], epoch_tc=t[1])
        # lr / kl_beta / free_bits / tc_weight: the effective values of the last completed step (eval:
        # always the full lr and beta, no floor and no penalty)
        st = dict(self._st_eval if eval else self._st)
        lr, kl = (self.hp["lr"], self.hp["kl_beta"]) if eval else self._effective(st["step"])
        st["lr"], st["kl_beta"] = float(lr), float(np.float32(kl))
        st["free_bits"] = 0.0 if eval else float(np.float32(self.hp["free_bits"]))
        st["tc_weight"] = 0.0 if eval else self._tc_effective(st["step"])
        return st

    def loss_history(self, eval: bool = False) -> np.ndarray:
        if self.state is not None:
            return self.state.loss_history(eval).numpy()
        return (self._hist_eval if eval else self._hist).copy()

    def _record(self, loss: float, eval: bool = False, tc: float = 0.0):
        """torch backend: what a step's kernels do to the device state -- the
        loss into its ring slot and the running sum, step and cursor advanced
        (the cursor wraps at nbatches)."""
        st, hist = (self._st_eval, self._hist_eval) if eval else (self._st, self._hist)
        hist[st["step"] % LOSS_HIST] = loss
        st["epoch_loss"] += loss
        st["epoch_tc"] += tc  # tc_batch of the step, unweighted (models/tc.py); the loss stays BCE + kl_t * KL
        st["epoch_count"] += 1
        st["step"] += 1
        st["cursor"] += 1
        if st["nbatches"] and st["cursor"] >= st["nbatches"]:
            st["cursor"] = 0

    def _torch_batch(self, X, idx, b: int, M: int, stream: int, step: int):
        """torch backend: rows ``X[idx[b*B : b*B + M]]`` and the step's noise."""
        rows = idx[b * self.B: b * self.B + M].long()
        eps = torch.from_numpy(reparam_eps(M, self.Z, self.seed, stream, step)).to(self.device)
        return X[rows], eps

    # graph-replayed passes (models/eval_graphs.py): the device buffers they read
    def _eval_state(self):
        return self.state.eval_state

    def _lat_hparams(self):
        return self.state.hparams

    # ------------------------------------------------------------------ data
    def _pad_index(self, idx: torch.Tensor):
        """``idx`` as a contiguous int32 device list padded to whole batches
        (the padding is never read: rows >= M) -> (idx, n, nbatches)."""
        idx = idx.to(device=self.device, dtype=torch.int32)
        n = idx.numel()
        nb = -(-n // self.B)
        pad = nb * self.B - n
        if pad:
            idx = torch.cat([idx, idx[:1].expand(pad)])
        return idx.contiguous(), n, nb

    def bind_train_data(self, X: torch.Tensor, idx: torch.Tensor):
        """X: [N, D] float32 on device; idx: int32 index list for the epoch."""
        assert X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] == self.D
        idx, n, nb = self._pad_index(idx)
        self._data = (X.contiguous(), idx, n, nb)
        self._graphs.clear()

    def train_data_changed(self):
        """The bound training rows were rewritten in place (same tensor, same
        index list: ``data/binarize.py``). Captured step graphs read the rows
        through the bound pointer at every replay and stay valid; a trainer
        that keeps rows gathered ahead of the step drops them here."""

    # ------------------------------------------------------------------ step
    def attach_reducer(self, reducer):
        """Reducer over ``self.grads`` whose bucket bounds come from ``bucket_bounds``."""
        self.reducer = reducer
        self._graphs.clear()
        from ..parallel.ddp import graph_capturable

        # a host-blocking (c10d/gloo) reducer cannot live inside a step graph: eager steps
        if not hasattr(self, "_graphs_wanted"):
            self._graphs_wanted = self.use_graphs
        self.use_graphs = self._graphs_wanted and graph_capturable(reducer)

    def default_bucket_bounds(self):
        return self.bucket_bounds(None)

    def train_steps(self, n: int, M: Optional[int] = None):
        """Run ``n`` training steps of ``M`` rows from the current cursor."""
        M = self.B if M is None else M
        if n <= 0:
            return
        self._not_averaged("train_steps")
        if self.backend == "torch":
            for _ in range(n):
                self._step_torch(M)
            return
        if not self.use_graphs:
            for _ in range(n):
                self._step_hip(M)
            return
        S = self.graph_steps
        while n >= S:
            self._replay(S, M)
            n -= S
        for _ in range(n):
            self._replay(1, M)

    def prepare(self, batch_sizes, eval_rows=None):
        """Set-up work done once before timing starts: capture the step graphs
        for the batch sizes an epoch uses and run the eval / decode kernels
        once (code-object load). Training state is left unchanged."""
        if self.backend != "hip":
            return
        if self.use_graphs and self._data is not None:
            for M in sorted({int(m) for m in batch_sizes if m and m > 0}):
                for S in {self.graph_steps, 1}:
                    if (S, M) not in self._graphs:
                        self._graphs[(S, M)] = self._capture(S, M)
        if eval_rows is not None and eval_rows.numel():
            st = self.read_state(eval=True)
            n = eval_rows.shape[0]
            self.evaluate(eval_rows, torch.arange(n, device=eval_rows.device, dtype=torch.int32))
            self.decode(torch.zeros(1, self.Z, device=self.device))
            self.set_cursor(st["cursor"], st["nbatches"], eval=True)
            self.reset_loss(eval=True)
        torch.cuda.synchronize(self.device)

    # strict_graphs: a replay that finds no captured graph raises instead of
    # capturing lazily (bench.py / autotune set it after ``prepare`` so no
    # capture ever lands inside a timed region)
    strict_graphs = False

    def _replay(self, S: int, M: int):
        key = (S, M)
        g = self._graphs.get(key)
        if g is None:
            if self.strict_graphs:
                raise RuntimeError(f"no captured step graph for (steps={S}, M={M}); call prepare() first")
            g = self._capture(S, M)
            self._graphs[key] = g
        g.replay()

    def _capture(self, S: int, M: int):
        # the warm-up and captured launches advance the step counter / cursor / Adam moments
        snap = (self.params, self.exp_avg, self.exp_avg_sq, self.state.train_state)
        return capture_replayable(snap + ((self.ema,) if self.ema_on else ()), lambda: self._step_hip(M), S)

    # ------------------------------------------------------------------ eval
    def evaluate(self, X: torch.Tensor, idx: torch.Tensor, want_first_recon: bool = True):
        """Forward + loss over (X[idx]); returns (sum_loss, recon of the first batch or None)."""
        idx, n, nb = self._pad_index(idx)
        X = X.contiguous()
        if self.backend == "hip" and self.use_graphs:
            first = self._eval_graphed(X, idx, n, want_first_recon)
            return self.read_state(eval=True)["epoch_loss"], first
        self.set_cursor(0, nb, eval=True)
        self.reset_loss(eval=True)
        first = None
        for b in range(nb):
            M = min(self.B, n - b * self.B)
            want = want_first_recon and b == 0
            if self.backend == "hip":
                self._eval_batch(M, X, idx, want)
                if want:
                    first = self._eval_recon(M)
            else:
                # -> (loss, recon [M, D] when wanted) of batch b at the eval step, with the full KL weight
                loss, recon = self._eval_batch_torch(X, idx, b, M, want)
                if want:
                    first = recon
                self._record(loss, eval=True)
        return self.read_state(eval=True)["epoch_loss"], first
