"""Convolutional VAE (28x28 and 128x128) on hand-written bf16 MFMA kernels.

North-star extension (BASELINE.json configs #2 and #5; absent from the
reference, whose model is the MLP of /root/reference/vae-hpo.py:19-45):
a conv/deconv encoder-decoder with the same ELBO (BCE(sum) + beta*KLD) and
reparameterisation as the reference.

Layout and precision: NHWC activations in bf16, fp32 master weights + fp32
gradients + fp32 Adam moments in flat arenas (one ``adam_cast`` launch per step
updates the masters and re-emits the bf16 weights AND their [Cin][KH][KW][Cout]
transposes), f32 accumulation everywhere, f32 mu/logvar/logits and loss.

Every layer maps onto the LDS-tiled implicit-GEMM kernels of
csrc/kernels/conv_igemm.hip (conv view: a convT is the conv whose backward-data
is its forward):
  conv    fwd = igemm(conv mode),   d_in = igemm(parity mode, Wt),  dW = wgrad(G=d_out, X=in)
  linear  = conv 1x1 on a 1x1 "image" (split-K when deep and narrow)
  convT   fwd = igemm(parity mode, Wt), d_in = igemm(conv mode),    dW = wgrad(G=in, X=d_out)
ReLU backward and the bias-gradient column sums are fused into the epilogue
that produces each gradient; weight gradients are m-split partial slabs that
one finalize launch reduces (deterministically) and feeds to a fused Adam.

The model definition and its torch oracle (``TorchConvVAE``) are in
conv_spec.py; the two step engines are mixins over this trainer's arenas:
conv_layers.py (layer by layer) and conv28.py (per-sample fused 28x28 step).
"""

from __future__ import annotations

import math
import os
from typing import Optional

import torch

from ..hpo.schedule import Schedule
from ..ops import native
from .conv28 import Fused28Step
from .conv_layers import LayerPathStep
from .conv_spec import Layer, TorchConvVAE, _w_shape, check_latent_size, conv_layout, conv_vae_spec
from .iw import iw_log_weights
from .mlp_vae import reference_adam_
from .trainer_base import EVAL_STREAM, VaeTrainerBase

__all__ = ["Layer", "conv_vae_spec", "TorchConvVAE", "ConvVaeTrainer", "conv_layout", "check_latent_size"]

GRAD_UNIT_WORDS = 12  # one GradUnit row (3 int32) of a uint8 finalize unit table, in its elements


class ConvVaeTrainer(Fused28Step, LayerPathStep, VaeTrainerBase):
    """One trial of the conv VAE. Same driver-facing API as MlpVaeTrainer."""

    def __init__(self, batch_size: int = 128, image: int = 28, channels: int = 1, z: int = 32, device=None,
                 backend: Optional[str] = None, seed: int = 0, lr: float = 1e-3, kl_beta: float = 1.0,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, decoupled_wd: bool = False,
                 rng_stream: int = 0, use_graphs: bool = True, graph_steps: int = 10, init_seed: Optional[int] = None,
                 schedule: Optional[Schedule] = None, free_bits: float = 0.0, tc_weight: float = 0.0,
                 ema_decay: float = 0.0):
        z = check_latent_size(z)
        super().__init__(batch_size, device, backend, seed, rng_stream, lr, kl_beta, betas, eps, weight_decay,
                         decoupled_wd, use_graphs, graph_steps, schedule,
                         dict(free_bits=free_bits, tc_weight=tc_weight, ema_decay=ema_decay))
        self.image, self.channels, self.Z = image, channels, z
        self.D = image * image * channels
        self.H = None
        self.spec = conv_vae_spec(image, channels, z)
        self.layout, self.numel = conv_layout(self.spec)
        # lookups that never change: encoder / decoder layers, layer by name, parameter name -> (offset, shape)
        self.enc = [l for l in self.spec if l.name.startswith("enc")]
        self.dec = [l for l in self.spec if l.name.startswith("dec")]
        self.by_name = {l.name: l for l in self.spec}
        self._param_at = {n: (o, s) for n, o, s in self.layout}
        # first decoder parameter: the default bucket boundary (decoder grads are ready first)
        self.split = self._param_at[self.dec[0].name + ".weight"][0]
        # horizontal fusion of independent backward launches (conv_jobs.hip);
        # MDT_CONV_JOBS=0 issues every op as its own kernel (A/B, bitwise equal)
        self.fuse_jobs = os.getenv("MDT_CONV_JOBS", "1") != "0"
        # finalize+Adam of each layer spread over the backward launches (third
        # job of the launch after its gradients completed) instead of all in
        # the optimizer tail (MDT_CONV_SPREAD_FIN, bitwise equal). Measured
        # neutral at 28x28 with the transposes in the tail (the tail shrinks,
        # the hosting launches grow by as much) and 0.7 % slower at 128x128
        # (profiles/r1_tail); with the transposes deferred (below) 1 % faster
        # at 28x28 (0.1208 -> 0.1196 ms, profiles/r1_defer). Round 4 (16-B
        # transposes, 64x32 shallow-Linear tiles) re-measured 128x128 B=64:
        # 0.3572-0.3585 spread vs 0.3595-0.3608 ms tail (profiles/r4_tiles):
        # on at every size now
        self.spread_fin = os.getenv("MDT_CONV_SPREAD_FIN", "1") == "1"
        # two-launch tail without the transposes (MDT_CONV_DEFER_WT=1|2, no
        # ticket, no fences): the tail's second launch is the first layer's
        # finalize alone, and the transposed weight copies ride in the next
        # step's first launch (=1) or in the decoder Linear's launch (=2: a
        # 50-block GEMM at 28x28 that leaves most CUs free for the copies).
        # Measured (profiles/r1_defer): 28x28 0.1249 -> 0.1232 (=1) -> 0.1209
        # ms/step (=2); 128x128 B=64 0.4517 -> 0.460 (=1) / 0.4545 (=2), so
        # the default is 2 up to 64x64 images and 0 above
        mode = os.getenv("MDT_CONV_DEFER_WT", "2" if image <= 64 else "0")
        self.defer_wt = mode in ("1", "2")
        self.wt_in_dec = mode == "2"
        self._init28()
        self._fused_launches = 0
        self._comm_packs = {}
        self._comm_tables = {}
        # profiling: int64 tensors ([grid][2] each) receiving per-workgroup start/end
        # stamps of the fused-reducer step's job launches (bench/ddp_structure.py); None = off
        self.comm_stamps = None
        # one-GPU multi-process rehearsals (eager only): push and reduce in separate
        # launches with ``comm_phase_hook()`` (e.g. device sync + host barrier)
        # between them, so no rank's reduce ever spins on a peer that shares
        # the GPU (tests/gpu/conv_ddp_worker.py)
        self.comm_split_tail = False
        self.comm_phase_hook = None
        # tests: the layer path's comm jobs leave the reduced gradients in `grads`, no update
        # (what f28_skip_adam is to the fused 28x28 step)
        self.comm_skip_adam = False
        torch.manual_seed(self.seed if init_seed is None else init_seed)
        ref = TorchConvVAE(self.spec, image, channels, z)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.numel, **f32)
        self.grads = torch.zeros(self.numel, **f32)
        self.exp_avg = torch.zeros(self.numel, **f32)
        self.exp_avg_sq = torch.zeros(self.numel, **f32)
        for name, t in ref.to_arena().items():
            self.named_parameters()[name].copy_(t)
        if self.backend == "torch":
            self.model = ref.to(self.device)
        else:
            self.C = native.require()
            self.state = self.C.TrialState(self.device.index or 0)
            self._alloc_hip()
        self._ema_alloc()
        self._push_hparams()

    # ----------------------------------------------------------- arenas
    def model_meta(self) -> dict:
        """Architecture record stored in checkpoints and validated on load."""
        return {"kind": "conv", "image": int(self.image), "channels": int(self.channels), "Z": int(self.Z),
                "layers": [[l.name, l.kind, l.cin, l.cout, l.k, l.s, l.p] for l in self.spec]}

    # ----------------------------------------------------------- state
    @property
    def comm_jobs(self) -> bool:
        """The step can host the fused all-reduce jobs (comm_jobs.h): the
        default intra-node reducer for this trainer is then kind "xgmi"."""
        return self.backend == "hip" and self.fuse_jobs

    def set_step(self, step):
        self._invalidate_prefetch()
        if self.backend == "hip":
            red = self.reducer
            if red is not None and hasattr(red, "rebase_epochs"):
                # the fused jobs' epoch is step + base: keep it increasing
                red.rebase_epochs(self.step_count, int(step))
        super().set_step(step)

    def set_cursor(self, cursor, nbatches, eval=False):
        if not eval:
            self._invalidate_prefetch()
        super().set_cursor(cursor, nbatches, eval)

    def bind_train_data(self, X, idx):
        super().bind_train_data(X, idx)
        self._invalidate_prefetch()
        self._plans28.clear()

    def train_data_changed(self):
        # the rows the last finalize gathered for the next step (f28_xn) are the old ones
        self._invalidate_prefetch()

    def attach_reducer(self, reducer):
        """Reducer over ``self.grads`` whose bucket bounds fall on layer starts
        (see ``bucket_bounds``); buckets launch as their layers' backward ends.
        A fused xGMI reducer (``XgmiP2PReducer(fused=True)``, kind "xgmi")
        instead contributes all-reduce JOBS to the step's own launches
        (csrc/kernels/comm_jobs.h): no second stream, no events."""
        super().attach_reducer(reducer)
        self._plans28.clear()
        self._comm_packs = {}
        self._comm_tables = {}

    def health_error(self) -> Optional[str]:
        """Silent-corruption check after an epoch (host sync): a paired-workgroup
        exchange of the fused 28x28 step that timed out (the step then trained on
        zero-filled partial sums, and an all-reduce would make the replicas agree
        on the corrupted gradient) or a reducer wait that gave up on a peer.
        None when healthy."""
        if self.backend != "hip":
            return None
        msgs = self._health28() if self.f28 else []
        red = self.reducer
        if red is not None and hasattr(red, "status"):
            st = int(red.status())
            if st:
                msgs.append(f"xGMI all-reduce gave up waiting for a peer (status {st})")
        return "; ".join(msgs) or None

    def _comm_ctx(self):
        """Device address of the fused reducer's CommCtx, or 0 (no reducer, or
        one that runs its collectives on its own stream)."""
        red = self.reducer
        if red is None or not hasattr(red, "comm_ctx") or not red.fused():
            return 0
        return int(red.comm_ctx())

    def _job(self, f):
        """A new job that ``f(job)`` recorded its launch into (conv_jobs.hip)."""
        j = self.C.Job()
        f(j)
        return j

    def _unit_args(self, segs, units, u0, u1):
        """Leading arguments of the arena kernels over finalize units [u0, u1) of a plan."""
        return (self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.w16, segs,
                units.narrow(0, u0 * GRAD_UNIT_WORDS, (u1 - u0) * GRAD_UNIT_WORDS), u1 - u0,
                self.state.train_state, self.state.hparams)

    def _grad_finalize(self, segs, units, u0, u1, adam, **kw):
        """Slab reduction into the gradient arena of finalize units [u0, u1);
        with ``adam`` also Adam and the bf16 cast. ``job=``: recorded, not launched."""
        self.C.grad_finalize(*self._unit_args(segs, units, u0, u1), adam, **kw)

    def _comm_job(self, segs, units, u0, u1, mode, adam, job=None):
        """A recorded all-reduce job over finalize units [u0, u1) of a plan
        (into ``job`` when given)."""
        j = self.C.Job() if job is None else job
        self.C.comm_job(*self._unit_args(segs, units, u0, u1), adam, self._comm_ctx(), mode, j)
        return j

    def _adam_cast(self, adam):
        """Every segment of the arenas in one launch: Adam when ``adam``, then
        the bf16 copies of the master weights."""
        h = self.state
        self.C.adam_cast(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.w16, self.segs, self.nseg,
                         h.train_state, h.hparams, adam)

    def layer_ranges(self):
        """[(layer, begin, end)] arena range of each layer's (weight, bias)."""
        at = self._param_at
        return [(l, at[l.name + ".weight"][0], at[l.name + ".bias"][0] + l.cout) for l in self.spec]

    def bucket_bounds(self, bucket_mb=None):
        """Bucket bounds in gradient-ready (reverse-layer) order, closed at layer
        boundaries once a bucket holds >= bucket_mb MiB of f32 gradients.
        None -> two buckets (decoder | encoder); 0 -> one bucket."""
        if bucket_mb == 0:
            return [0, self.numel]
        if bucket_mb is None:
            return [0, self.split, self.numel]
        cap = float(bucket_mb) * (1 << 20)
        bounds, acc = [self.numel], 0.0
        for l, b, e in reversed(self.layer_ranges()):
            acc += 4.0 * (e - b)
            if acc >= cap and b > 0:
                bounds.append(b)
                acc = 0.0
        bounds.append(0)
        return sorted(set(bounds))

    @torch.no_grad()
    def refresh_weights(self):
        """Re-derive the bf16 compute copies after ``params`` changed outside a
        step (replica broadcast, checkpoint load)."""
        if self.backend == "hip":
            self._cast_weights()
            self._wt_stale = False  # the cast is followed by every layer's transposed copy
        else:
            self.model.from_arena(self.named_parameters())

    def _refresh_swapped(self):
        """``averaged_weights()`` exchanged params and ema: ``refresh_weights()``
        with the transposed copies a step keeps current (layers 1 .., as
        ``_wtrans_layers`` in the step; the first layer's copy is never read and
        stays as it was), so that after the context ``w16`` and ``w16t`` are
        bitwise what they were before it."""
        if self.backend != "hip":
            self.refresh_weights()
            return
        self._adam_cast(False)
        self._wtrans_layers(1, len(self.spec))
        self._wt_stale = False

    # ----------------------------------------------------------- HIP path
    def _alloc_hip(self):
        dev, B = self.device, self.B
        bf = dict(dtype=torch.bfloat16, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.w16 = torch.zeros(self.numel, **bf)
        toff, self._toff = 0, {}
        for l in self.spec:
            self._toff[l.name] = toff
            toff = (toff + math.prod(_w_shape(l)) + 63) // 64 * 64
        self.w16t = torch.zeros(max(toff, 64), **bf)
        rows = self._seg_rows({})
        self.segs = self.C.make_grad_segs(rows, dev.index or 0)
        self.nseg = 2 * len(self.spec)
        tr = []
        self._tr_layer = []  # layer li owns transpose units [_tr_layer[li], _tr_layer[li + 1])
        for si, r in enumerate(rows):
            if si % 2 == 0:
                self._tr_layer.append(len(tr))
            if r[8] < 0:
                continue
            co, k, ci = r[4], r[5], r[7]
            for tap in range(k * k):
                for co0 in range(0, co, 64):
                    for ci0 in range(0, ci, 64):
                        tr.append([si, tap, co0, ci0])
        self._tr_layer.append(len(tr))
        self.tr_units = self.C.make_tr_units(tr, dev.index or 0)
        self.xb = torch.zeros(B, self.D, **f32)
        self.acts, self.gacts = {}, {}
        for l in self.spec:
            n_out = B * l.out_hw * l.out_hw * l.cout
            self.acts[l.name] = torch.zeros(n_out, **bf)
            self.gacts[l.name] = torch.zeros(n_out, **bf)
        zf = self.Z
        self.mulv = torch.zeros(B, 2 * zf, **f32)
        self.eps = torch.zeros(B, zf, **f32)
        self.z16 = torch.zeros(B, zf, **bf)
        self.dz = torch.zeros(B, zf, **f32)
        self.dmulv = torch.zeros(B, 2 * zf, **f32)
        self.dmulv16 = torch.zeros(B, 2 * zf, **bf)
        if self.tc_on:
            self._tc_alloc()
        self.logits = torch.zeros(B * self.D, **f32)
        self.recon = torch.zeros(B * self.D, **f32)
        self.dlog16 = torch.zeros(B * self.D, **bf)
        first, last = self.spec[0], self.spec[-1]
        # single-channel edge layers run on the direct kernels of conv_thin.hip
        self._thin_first = first.kind == "conv" and first.cin == 1 and first.cout in (16, 32, 64) and first.k <= 4
        self._thin_last = (last.kind == "convT" and last.cout == 1 and last.cin in (16, 32, 64) and last.k % last.s == 0
                           and last.out_hw % last.s == 0)
        self.bce_part = torch.zeros(max(self._n_bce(B), 1), **f32)
        self.kld_part = torch.zeros(B * zf, **f32)  # >= KLD partials of reparam / combine_reparam
        self._plans = {}
        if self.f28:
            self._alloc28()
        self._cast_weights()

    def _seg_rows(self, slabs):
        """GradSeg rows (off, numel, slab_ptr, nsplit, co, k, s, ci, toff) for every
        weight and bias; ``slabs`` maps a parameter name to (tensor, nsplit)."""
        rows = []
        for l in self.spec:
            for suffix in (".weight", ".bias"):
                name = l.name + suffix
                o, shp = self._param_at[name]
                t, ns = slabs.get(name, (None, 1))
                ptr = t.data_ptr() if t is not None else 0
                if suffix == ".weight":
                    rows.append([o, math.prod(shp), ptr, ns, shp[0], shp[1], l.s, shp[3], self._toff[l.name]])
                else:
                    rows.append([o, shp[0], ptr, ns, 0, 0, 0, 0, -1])
        return rows

    @staticmethod
    def _finalize_units(segs):
        """GradUnit rows (seg, start, count) of the finalize kernel for GradSeg
        rows ``segs``; layer i owns units [layer_units[i], layer_units[i+1])."""
        units, layer_units = [], []
        for si, (off, numel, ptr, ns, *_rest) in enumerate(segs):
            if si % 2 == 0:
                layer_units.append(len(units))
            rp = 1  # partial rows per unit column; 256-thread finalize blocks (kFinalizeThreads)
            if ptr:
                while rp < 256 and rp * 16 < ns:
                    rp *= 2
            cnt = 256 // rp
            if rp == 1 and numel % 4 == 0 and off % 4 == 0 and ptr % 16 == 0:
                cnt = 4 * 256  # grad_finalize_vec4: 4 elements per thread, 16-B accesses
            for st in range(0, numel, cnt):
                units.append([si, st, min(cnt, numel - st)])
        layer_units.append(len(units))
        return units, layer_units

    def _cast_weights(self):
        self._adam_cast(False)
        self._transpose_weights()

    def _transpose_weights(self):
        """bf16 weights -> parity-ordered transposed copies (one coalesced launch)."""
        self._wtrans_layers(0, len(self.spec))

    def _weight_of(self, arena, l):
        o, s = self._param_at[l.name + ".weight"]
        return arena.narrow(0, o, math.prod(s))

    def _wf32(self, l):
        """f32 master weight of a layer (read directly by the thin kernels)."""
        return self._weight_of(self.params, l)

    def _w(self, l):
        return self._weight_of(self.w16, l)

    def _wt(self, l):
        s = _w_shape(l)
        return self.w16t.narrow(0, self._toff[l.name], math.prod(s))

    def _b(self, l):
        return self.named_parameters()[l.name + ".bias"]

    def _gw(self, l):
        return self._weight_of(self.grads, l)

    def _gb(self, l):
        return self.named_grads()[l.name + ".bias"]

    @staticmethod
    def _desc(l: Layer, M: int):
        if l.kind == "convT":  # conv geometry: conv input = convT output
            return [M, l.out_hw, l.out_hw, l.cout, l.in_hw, l.in_hw, l.cin, l.k, l.k, l.s, l.p]
        return [M, l.in_hw, l.in_hw, l.cin, l.out_hw, l.out_hw, l.cout, l.k, l.k, l.s, l.p]

    def _step_hip(self, M):
        # weight averaging: ema_update is the last launch of every step form -- the layer path's
        # optimizer tail, the fused 28x28 step's finalize, adam_cast after a reducer, both comm-job tails
        (self._step28 if self.f28 else self._step_layers)(M)
        self._ema_step_hip()

    # ----------------------------------------------------------- torch path
    def _step_torch(self, M):
        X, idx = self._data[0], self._data[1]
        st = self._st
        x, eps = self._torch_batch(X, idx, st["cursor"], M, self.rng_stream, st["step"])
        self.model.zero_grad(set_to_none=True)
        lr_t, kl_t = self._effective(st["step"] + 1)
        loss, _, mu, lv = self.model.loss(x, eps, kl_t, self.hp["free_bits"])
        tc = 0.0
        if self.tc_on:
            # the objective also carries tc_t * tc_batch (models/tc.py); the recorded loss stays BCE + kl_t * KL
            from .tc import tc_batch

            tcb = tc_batch(mu, lv, eps)
            tc = float(tcb.detach())
            (loss + self._tc_effective(st["step"] + 1) * tcb).backward()
        else:
            loss.backward()
        with torch.no_grad():
            gv = self.named_grads()
            for k, v in self.model.grads_to_arena().items():
                gv[k].copy_(v)
            if self.reducer is not None:
                self.reducer.launch_all()
                self.reducer.wait_all()
            h = self.hp
            reference_adam_(self.params, self.grads, self.exp_avg, self.exp_avg_sq, st["step"] + 1, lr_t,
                            h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["grad_scale"], self.decoupled_wd)
            self.model.from_arena(self.named_parameters())
            self._ema_step_torch(st["step"] + 1)
        self._record(float(loss.detach()), tc=tc)

    # ----------------------------------------------------------- driver API
    def train_steps(self, n, M=None):
        super().train_steps(n, M)
        if n > 0 and self.backend == "hip" and (self._wt_deferred() or self.f28):
            # the last step's transposed weight copies (deferred to the next
            # step's first launch, or never needed by the fused 28x28 step) are
            # stale now: eval / decode write them first (_ensure_wt)
            self._wt_stale = True

    _wt_stale = False

    def _ensure_wt(self):
        """Write the transposed weight copies (w16t) if training left them
        stale. Only eval / decode read them outside a training step: a step of
        the layer path writes its own in its first launch, and the fused 28x28
        step never reads them."""
        if self._wt_stale:
            self._wtrans_layers(1, len(self.spec))
            self._wt_stale = False

    def _capture(self, S, M):
        red = self.reducer
        k0 = self.step_count if red is not None and hasattr(red, "rebase_epochs") else None
        g = super()._capture(S, M)
        if k0 is not None:
            # the warm-up step ran the fused all-reduce jobs at epoch k0 + 1 and
            # published flags for it; the step counter now goes back to k0, so
            # the next real step must not reuse that epoch (every member
            # captures at the same points: the rebase is the same everywhere)
            red.rebase_epochs(k0 + 1, k0)
        self._cast_weights()
        return g

    @torch.no_grad()
    # graph-replayed eval passes (models/eval_graphs.py)
    def _eval_batch(self, M, X, idx, want_recon):
        if self.f28:
            self._eval_batch28(M, X, idx, want_recon)
            return
        st = self.state
        self._forward_hip(M, st.eval_state, EVAL_STREAM + self.rng_stream, want_recon=want_recon, train=False,
                          src=(X, idx))
        self.C.loss_finalize2(self.bce_part, self._n_bce(M), self.kld_part, self._n_kld(M), st.eval_state,
                              st.hparams, True)

    def _eval_recon(self, M):
        return self.recon[: M * self.D].view(M, self.D).clone()

    def _eval_batch_torch(self, X, idx, b, M, want_recon):
        x, eps = self._torch_batch(X, idx, b, M, EVAL_STREAM + self.rng_stream, self._st_eval["step"])
        loss, t, _, _ = self.model.loss(x, eps, self.hp["kl_beta"])
        recon = torch.sigmoid(t).permute(0, 2, 3, 1).reshape(M, self.D).clone() if want_recon else None
        return float(loss.detach()), recon

    def evaluate(self, X, idx, want_first_recon=True):
        self._ensure_wt()
        return super().evaluate(X, idx, want_first_recon)

    # importance-weighted log-likelihood pass (models/eval_graphs.py::GraphedIwEval.evaluate_iw)
    def _iw_logw_torch(self, x, eps):
        mu, lv = self.model.encode(x)
        dec = lambda z: self.model.decode_logits(z).permute(0, 2, 3, 1).reshape(z.shape[0], self.D)
        return iw_log_weights(mu, lv, eps, x, dec)[0]

    def _iw_prepare(self):
        self._ensure_wt()  # the decoder's parity-mode layers read the transposed copies, as in evaluate() / decode()
        if getattr(self, "iw_state", None) is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            self.iw_state = self.C.iw_state_new(self.device.index or 0)
            self.iw_eps = torch.zeros(self.B, self.Z, **f32)
            self.iw_z = torch.zeros(self.B, self.Z, **f32)
            self.iw_prior = torch.zeros(self.B, **f32)
            self.iw_bce = torch.zeros(self.B, **f32)
            self.iw_rowbuf = torch.zeros(3, self.B, **f32)

    def _iw_begin(self, nbatches):
        self.C.iw_state_begin(self.iw_state, nbatches)

    def _iw_batch(self, M, X, idx, k, S, rows):
        """One batch at the pass cursor: the layer-path encoder once (also at
        28x28: the fused forward cannot emit K decodes), then the samples in
        chunks of at most B virtual rows v = s*M + i through the decoder layers
        exactly as ``decode()`` runs them, the per-row BCE and the shared
        reduce kernel (which advances the pass cursor after the last chunk)."""
        C, st, hp = self.C, self.iw_state, self.state.hparams
        self._forward_hip(M, st, 0, train=False, src=(X, idx), enc_only=True)
        Sc = max(1, min(S, self.B // M))
        for k0 in range(0, k, Sc):
            s = min(Sc, k - k0)
            V = s * M
            C.iw_reparam(self.mulv, M, self.B, self.Z, k0, s, st, hp, self.z16, self.iw_z, self.iw_eps, self.iw_prior)
            self._decode_z16(V)
            C.iw_row_bce(self.logits, self.xb, V, M, self.D, self.iw_bce)
            C.iw_reduce(self.iw_prior, self.iw_bce, self.iw_rowbuf, rows[0], rows[1], st, M, self.B, k, s,
                        k0 == 0, k0 + s >= k)

    def _iw_state(self):
        return self.iw_state

    def _iw_ws_token(self):
        return 0  # fixed-size buffers (a chunk holds at most B virtual rows)

    def _iw_read(self):
        r = self.C.iw_state_read(self.iw_state)
        return r[0], r[1]

    def iw_buffers(self, S: int, M: int):
        """hip backend: ``mulv[M, 2Z]`` of the last batch of the last
        ``evaluate_iw`` pass and ``eps`` / ``z`` ``[S, M, Z]`` (f32, before the
        decoder's bf16 rounding) of its last chunk of S samples (copies)."""
        n = S * M
        return dict(mulv=self.mulv[:M].clone(), eps=self.iw_eps.view(-1)[: n * self.Z].view(S, M, self.Z).clone(),
                    z=self.iw_z.view(-1)[: n * self.Z].view(S, M, self.Z).clone())

    # latent report pass (models/eval_graphs.py::GraphedLatentEval.evaluate_latent)
    def _lat_encode_torch(self, x):
        return self.model.encode(x)

    def _lat_prepare(self):
        self._ensure_wt()
        if getattr(self, "latent_state", None) is None:
            self.latent_state = self.C.latent_state_new(self.device.index or 0)

    def _lat_begin(self, nbatches):
        self.C.latent_state_begin(self.latent_state, nbatches)

    def _lat_batch(self, M, X, idx, rows):
        """One batch at the pass cursor: the layer-path encoder as in
        ``_iw_batch`` (it begins the step on the pass state), then the collect
        kernel files ``mulv[:M]`` into the pass buffer and advances the cursor."""
        self._forward_hip(M, self.latent_state, 0, train=False, src=(X, idx), enc_only=True)
        self.C.latent_collect(self.mulv, M, self.B, self.Z, rows, self.latent_state)

    def _lat_state(self):
        return self.latent_state

    @torch.no_grad()
    def decode(self, zz):
        zz = zz.to(self.device, torch.float32)
        if self.backend == "torch":
            t = self.model.decode_logits(zz)
            return torch.sigmoid(t).permute(0, 2, 3, 1).reshape(zz.shape[0], self.D)
        self._ensure_wt()
        outs = []
        for i in range(0, zz.shape[0], self.B):
            zc = zz[i:i + self.B]
            M = zc.shape[0]
            self.z16[:M].copy_(zc.to(torch.bfloat16))
            self._decode_z16(M)
            outs.append(torch.sigmoid(self.logits[: M * self.D].view(M, self.D)).clone())
        return torch.cat(outs)

    def flops_per_sample(self):
        f = 0
        for l in self.spec:
            f += 2 * l.out_hw * l.out_hw * l.cout * l.k * l.k * l.cin if l.kind != "convT" else \
                2 * l.in_hw * l.in_hw * l.cin * l.k * l.k * l.cout
        return 3 * f
