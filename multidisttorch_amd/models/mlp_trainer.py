"""One HPO trial's MLP-VAE training state and step, on the fused HIP path or
the torch reference path.

Replaces the reference's per-step chain (DataLoader collate -> H2D copy ->
DDP forward -> loss -> autograd backward -> DDP bucket all-reduce ->
``loss.item()`` sync -> foreach Adam; /root/reference/vae-hpo.py:67-74) with:

* ``backend="hip"``: ``_C.MlpVaeEngine`` — seven fused CDNA4 launches per step
  (csrc/kernels/vae_mlp.hip, adam.hip) reading the batch rows straight out of
  a device-resident dataset through the epoch's sampler index list, gradient
  buckets all-reduced by the native ``BucketReducer`` while later backward
  kernels run, and the whole step (optionally S steps) captured in one
  hipGraph and replayed; the loss stays on the device (ring buffer) and is
  read at log points only.
* ``backend="torch"``: the same math in torch ops (``reference_step``), used on
  CPU hosts and as the fp32 oracle for the kernel tests.

Both backends share the flat-arena layout, the Philox noise stream and Adam
arithmetic, so a run is reproducible across them up to fp32 rounding.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

from ..hpo.schedule import Schedule
from ..ops import native
from .iw import mlp_encode, mlp_iw_log_weights
from .mlp_vae import arena_layout, init_params_, reference_adam_, reference_forward, reference_step
from .trainer_base import EVAL_STREAM, VaeTrainerBase

__all__ = ["MlpVaeTrainer"]


class MlpVaeTrainer(VaeTrainerBase):
    def __init__(self, batch_size: int = 128, D: int = 784, H: int = 400, Z: int = 20,
                 device=None, backend: Optional[str] = None, seed: int = 0, init_seed: Optional[int] = None,
                 lr: float = 1e-3, kl_beta: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled_wd: bool = False, rng_stream: int = 0,
                 use_graphs: bool = True, graph_steps: int = 10, schedule: Optional[Schedule] = None,
                 free_bits: float = 0.0, tc_weight: float = 0.0, ema_decay: float = 0.0):
        super().__init__(batch_size, device, backend, seed, rng_stream, lr, kl_beta, betas, eps, weight_decay,
                         decoupled_wd, use_graphs, graph_steps, schedule,
                         dict(free_bits=free_bits, tc_weight=tc_weight, ema_decay=ema_decay))
        self.D, self.H, self.Z = D, H, Z
        self.layout, self.numel, self.split = arena_layout(D, H, Z)
        if self.backend == "hip":
            C = native.require()
            self.engine = C.MlpVaeEngine(batch_size, D, H, Z, self.device.index or 0)
            self.state = self.engine.state
            lay = [(n, o, tuple(s)) for n, o, s in self.engine.layout()]
            assert sorted(lay) == sorted(self.layout) and self.engine.numel() == self.numel, \
                "C++/Python arena layouts disagree"
            self.params, self.grads = self.engine.params, self.engine.grads
            self.exp_avg, self.exp_avg_sq = self.engine.exp_avg, self.engine.exp_avg_sq
            if self.tc_on:
                # the penalty's kernels write their share of d[mu|lv] here and B2 adds it (vae_tc.hip)
                self._tc_alloc()
                self.engine.set_dmulv_add(self.tc_add)
        else:
            self.engine = None
            z = lambda: torch.zeros(self.numel, dtype=torch.float32, device=self.device)
            self.params, self.grads, self.exp_avg, self.exp_avg_sq = z(), z(), z(), z()
        g = torch.Generator().manual_seed(self.seed if init_seed is None else int(init_seed))
        host = torch.zeros(self.numel, dtype=torch.float32)
        init_params_(host, self.layout, g)
        self.params.copy_(host)
        self._ema_alloc()
        self._push_hparams()

    def bucket_bounds(self, bucket_mb=None):
        """The fused step finishes gradients in two groups (fc4 after B2,
        the rest after B3): two buckets, or one when bucket_mb == 0."""
        return [0, self.numel] if bucket_mb == 0 else [0, self.split, self.numel]

    # measured cost (us per step) of splitting the MLP backward around a
    # side-stream bucket launch, per reducer family: overlap minus inline with
    # forced one-rank collectives, 77.5 - 56.9 (RCCL) and 81.9 - 68.0 (p2p
    # kernel) on a 49.0 us step (profiles/r4_ddp_fused/ddp_structure_mlp.json)
    SPLIT_COST_US = {"rccl": 20.5, "p2p": 14.0}

    def _overlap(self) -> bool:
        red = self.reducer
        if red is None or red.num_buckets() != 2:
            return False
        if self.ddp_overlap is not None:
            return bool(self.ddp_overlap)
        from ..parallel.ddp import overlap_pays

        fam = "rccl" if type(red).__name__.startswith("Rccl") else "p2p"
        return overlap_pays(4 * (self.numel - self.split), self.SPLIT_COST_US[fam])

    def _step_hip(self, M: int):
        self._step_hip_raw(M)
        self._ema_step_hip()  # weight averaging: the last launch of the step, after either Adam form

    def _step_hip_raw(self, M: int):
        X, idx = self._data[0], self._data[1]
        e = self.engine
        e.forward(X, idx, M, True, False, self.rng_stream, False)
        self._tc_step(M)
        early = self._overlap()
        if self.reducer is not None and hasattr(self.reducer, "set_inline"):
            self.reducer.set_inline(not early)
        if early:
            e.backward(X, idx, M, 1, False)
            e.backward(X, idx, M, 2, False)
            self.reducer.launch(1)          # fc4 bucket (final after B2): overlaps B3
            e.backward(X, idx, M, 3, False)
            self.reducer.launch(0)
            self.reducer.wait_all()
            e.adam()
        elif self.reducer is not None:      # every bucket after the whole backward
            e.backward(X, idx, M, 0, False)
            for k in reversed(range(self.reducer.num_buckets())):
                self.reducer.launch(k)
            self.reducer.wait_all()
            e.adam()
        else:
            # Adam fused into the weight-gradient epilogues of B3
            e.backward(X, idx, M, 0, True)

    def _tc_step(self, M: int):
        """Between forward and backward of a training step: value and gradient
        of tc_t * tc_batch from the step's mulv and eps (csrc/kernels/vae_tc.hip),
        into the buffer B2 adds to d[mu|lv]. Nothing without the penalty."""
        if self.tc_on:
            e = self.engine
            native.require().tc_penalty(e.act("mulv", M), e.act("eps", M), M, self.Z, self.tc_ws, self.tc_value,
                                        state=self.state.train_state, add_out=self.tc_add)

    _CPU_ORDER = ("fc1.weight", "fc1.bias", "fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias",
                  "fc3.weight", "fc3.bias", "fc4.weight", "fc4.bias")

    def _cpu_native(self):
        """The fused native CPU step (csrc/runtime/cpu_mlp.cpp) when the torch
        backend runs on the host and the extension is built; None otherwise
        (stock torch ops, ``reference_step``)."""
        if self.device.type != "cpu" or not native.available() or self.tc_on:
            return None  # the total-correlation penalty runs on the stock-torch path
        if getattr(self, "_cpu", None) is None:
            self._cpu = native.require().MlpCpuStep(self.B, self.D, self.H, self.Z)
            v, g = self.named_parameters(), self.named_grads()
            self._cpu_w = [v[n] for n in self._CPU_ORDER]
            self._cpu_g = [g[n] for n in self._CPU_ORDER]
        return self._cpu

    @torch.no_grad()
    def _step_torch(self, M: int):
        X, idx = self._data[0], self._data[1]
        st = self._st
        h = self.hp
        lr_t, kl_t = self._effective(st["step"] + 1)
        cpu = self._cpu_native()
        if cpu is not None:
            loss = cpu.forward_backward(self._cpu_w, self._cpu_g, X, idx, st["cursor"] * self.B, M, self.seed,
                                        self.rng_stream, st["step"], kl_t, free_bits=h["free_bits"])
        else:
            x, eps = self._torch_batch(X, idx, st["cursor"], M, self.rng_stream, st["step"])
            f = reference_step(self.named_parameters(), self.named_grads(), x, eps, kl_t,
                               free_bits=h["free_bits"],
                               tc_t=self._tc_effective(st["step"] + 1) if self.tc_on else None)
            loss = None
        if self.reducer is not None:
            self.reducer.launch(1)
            self.reducer.launch(0)
            self.reducer.wait_all()
        if cpu is not None:
            cpu.adam(self.params, self.grads, self.exp_avg, self.exp_avg_sq, st["step"] + 1, lr_t, h["beta1"],
                     h["beta2"], h["eps"], h["weight_decay"], h["grad_scale"], self.decoupled_wd)
        else:
            reference_adam_(self.params, self.grads, self.exp_avg, self.exp_avg_sq, st["step"] + 1,
                            lr_t, h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["grad_scale"],
                            self.decoupled_wd)
            loss = float(f["loss"])
        self._ema_step_torch(st["step"] + 1)
        self._record(loss, tc=float(f["tc_batch"]) if cpu is None and self.tc_on else 0.0)

    def model_meta(self) -> dict:
        """Architecture record stored in checkpoints and validated on load."""
        return {"kind": "mlp", "D": int(self.D), "H": int(self.H), "Z": int(self.Z)}

    # ------------------------------------------------------------------ eval / sample
    @torch.no_grad()
    # graph-replayed eval passes (models/eval_graphs.py)
    def _eval_batch(self, M, X, idx, want_recon):
        self.engine.forward(X, idx, M, False, True, EVAL_STREAM + self.rng_stream, want_recon)
        self.engine.loss_finalize(True)

    def _eval_recon(self, M):
        return self.engine.act("recon", M).clone()

    def _eval_batch_torch(self, X, idx, b, M, want_recon):
        step, beta = self._st_eval["step"], self.hp["kl_beta"]
        cpu = self._cpu_native()
        if cpu is not None:  # fused native forward + loss (csrc/runtime/cpu_mlp.cpp)
            loss = cpu.forward_backward(self._cpu_w, self._cpu_g, X, idx, b * self.B, M, self.seed,
                                        EVAL_STREAM + self.rng_stream, step, beta, backward=False)
            return loss, cpu.recon() if want_recon else None
        x, eps = self._torch_batch(X, idx, b, M, EVAL_STREAM + self.rng_stream, step)
        f = reference_forward(self.named_parameters(), x, eps, beta)
        return float(f["loss"]), f["p"].clone() if want_recon else None


    # importance-weighted log-likelihood pass (models/eval_graphs.py::GraphedIwEval.evaluate_iw)
    def _iw_logw_torch(self, x, eps):
        return mlp_iw_log_weights(self.named_parameters(), x, eps)[0]

    def _iw_prepare(self):
        pass

    def _iw_begin(self, nbatches):
        self.engine.iw_begin(nbatches)

    def _iw_batch(self, M, X, idx, k, S, rows):
        # encoder once (F1), then per chunk: sample, decoder + per-row BCE, reduce (csrc/kernels/vae_iw.hip)
        self.engine.iw_batch(X, idx, M, k, S, rows[0], rows[1])

    def _iw_state(self):
        return self.engine.iw_state

    def _iw_ws_token(self):
        return self.engine.iw_capacity()  # the engine's chunk workspace grows with chunk_samples

    def _iw_read(self):
        r = self.engine.iw_read()
        return r[0], r[1]

    def iw_buffers(self, S: int, M: int) -> Dict[str, torch.Tensor]:
        """hip backend: ``mulv[M, 2Z]`` of the last batch of the last
        ``evaluate_iw`` pass and ``eps`` / ``z`` ``[S, M, Z]`` of its last chunk
        of S samples (copies)."""
        e = self.engine
        return dict(mulv=e.act("mulv", M).clone(), eps=e.iw_act("eps", S, M).clone(), z=e.iw_act("z", S, M).clone())

    # latent report pass (models/eval_graphs.py::GraphedLatentEval.evaluate_latent)
    def _lat_encode_torch(self, x):
        return mlp_encode(self.named_parameters(), x)

    def _lat_prepare(self):
        pass

    def _lat_begin(self, nbatches):
        self.engine.latent_begin(nbatches)

    def _lat_batch(self, M, X, idx, rows):
        # encoder (F1) on the pass state, the slab sum to mulv, the rows into the pass buffer
        self.engine.latent_batch(X, idx, M, rows)

    def _lat_state(self):
        return self.engine.latent_state

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        z = z.to(self.device, torch.float32).contiguous()
        if self.backend == "hip":
            out = []
            for i in range(0, z.shape[0], self.B):
                out.append(self.engine.decode(z[i:i + self.B].contiguous()))
            return torch.cat(out)
        v = self.named_parameters()
        h3 = torch.relu(z @ v["fc3.weight"].t() + v["fc3.bias"])
        return torch.sigmoid(h3 @ v["fc4.weight"].t() + v["fc4.bias"])

    # ------------------------------------------------------------------ info
    def flops_per_sample(self) -> float:
        D, H, Z = self.D, self.H, self.Z
        fwd = D * H + H * 2 * Z + Z * H + H * D
        bwd = 2 * fwd - D * H  # no dX for the input layer
        return 2.0 * (fwd + bwd)
