"""Per-sample fused 28x28 step engine of ``ConvVaeTrainer`` (a mixin over the
trainer's arenas, weight views and buffers, models/conv_vae.py) in its solo,
RCCL-bucket and fused-xGMI forms. What the fused step owns is set up by
``_init28`` (switches) and ``_alloc28`` (device buffers)."""

import math
import os

import torch

from ..ops.conv_plans import wgrad_plan
from .conv_spec import _w_shape
from .trainer_base import EVAL_STREAM


class Fused28Step:
    def _init28(self):
        # per-sample fused 28x28 step (csrc/kernels/conv28_fused.hip): forward,
        # backward-data, weight gradients and optimizer in 4 launches instead of
        # the layer-by-layer path's 15. MDT_CONV_F28=0 keeps the layer path.
        # The fused step owns a sample end to end in one workgroup pair and cannot host
        # a cross-sample term: a trainer with the total-correlation penalty trains on
        # the layer path (which already serves 28x28 for z != 32).
        self.f28 = (self.backend == "hip" and self.image == 28 and self.channels == 1 and self.Z == 32
                    and os.getenv("MDT_CONV_F28", "1") != "0" and not self.tc_on)
        self._plans28 = {}
        self.f28_skip_adam = False  # tests: leave the reduced gradients in `grads`, no update
        # forward and backward of the fused step in one launch (MDT_F28_MERGE=0: two)
        self.f28_merge = os.getenv("MDT_F28_MERGE", "1") != "0"
        # the merged step with two workgroups per sample (conv28_pair.h): a
        # B = 128 trial fills all 256 CUs instead of 128. MDT_F28_PAIR=0 (A/B): one per sample
        self.f28_pair = os.getenv("MDT_F28_PAIR", "1") != "0"
        # eval passes through the same paired form, forward only (MDT_F28_EVAL_PAIR=0: solo f28_fwd_k)
        self._eval_pair = os.getenv("MDT_F28_EVAL_PAIR", "1") != "0"
        # tests: > 0 delays every partner workgroup (forces the solo fallback); < 0 stalls sample 0's
        # role-1 half after pairing (forces an exchange timeout: f28_err, health_error());
        # MDT_F28_TEST_STALL_US=N sets -N (fault drills through the HPO runner / bench)
        self.f28_pair_delay_us = -int(os.getenv("MDT_F28_TEST_STALL_US", "0"))
        # profiling: int64 [B*16] tensors (fwd, bwd) receiving per-workgroup
        # phase-end s_memrealtime stamps (obs/f28_phases.py); None = off
        self.f28_stamps = (None, None)

    def _alloc28(self):
        """Device state of the fused step (``self.f28`` trainers only)."""
        B, dev = self.B, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.dlog32 = torch.zeros(B * self.D, **f32)
        self.f28_part = torch.zeros(3 * B, **f32)                  # bce | kld | dec2-bias partials
        # bias partials: dec_fc [B][3136] | dec1 [B][32] | enc2 [2][B][64] (a row per pair half) | enc1 [B][32]
        self.f28_bias = torch.zeros(B * (3136 + 32 + 128 + 32), **f32)
        # paired step state: exchange granules, pairing words, error word (all zero between launches)
        self.f28_xg = torch.zeros(B * 2 * self.C.f28_pair_words(), dtype=torch.int64, device=dev)
        self.f28_pairw = torch.zeros(B, dtype=torch.int32, device=dev)
        self.f28_err = torch.zeros(1, dtype=torch.int32, device=dev)
        # next-batch prefetch: the finalize of step k gathers step k+1's rows
        # into f28_xn and tags them with the step they are for (f28_xtag);
        # -1 = nothing gathered (the host invalidates on cursor/data/step moves)
        self.f28_xn = torch.zeros(B * self.D, **f32)
        self.f28_xtag = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.f28_prefetch = os.getenv("MDT_F28_PREFETCH", "1") != "0"
        # MDT_F28_EPI_ADAM=1: the two single-split Linear weight gradients
        # (enc_head, dec_fc: 81 % of the parameters) apply Adam in their
        # epilogues and write no partial slab; the finalize launch loses
        # their units. The step kernel hands the step's Adam constants over
        # in f28_adamc (adam_common.h adam_consts_next). Bitwise the
        # two-launch tail (tests/gpu/test_f28_epilogue_adam.py)
        self.f28_epi_adam = os.getenv("MDT_F28_EPI_ADAM", "1") != "0"
        self.f28_adamc = torch.zeros(16, **f32)  # one AdamC (64 B), rewritten by every training launch

    def _invalidate_prefetch(self):
        """The host moved the cursor, the step or the data: rows the last
        finalize gathered are not the next step's (f28 P0 falls back to the
        index chain until the next finalize gathers again)."""
        xt = getattr(self, "f28_xtag", None)
        if xt is not None:
            xt.fill_(-1)

    def _health28(self):
        """The fused step's share of ``health_error()`` (host sync): messages."""
        msgs = []
        err = int(self.f28_err.item())
        if err:
            msgs.append(f"fused 28x28 step: a paired-workgroup exchange timed out (f28_err={err}); "
                        f"the trial trained on incomplete partial sums")
        return msgs

    def _plan28(self, M):
        """Tensor tables, weight-gradient jobs and finalize units of the fused
        28x28 step for a batch of M (built once per M and data binding; the
        tensors never move, so captured graphs stay valid)."""
        p = self._plans28.get(M)
        if p is not None:
            return p
        C, dev, B = self.C, self.device, self.B
        f32 = dict(dtype=torch.float32, device=dev)
        X, idx = self._data[0], self._data[1]
        st = self.state
        bce, kld, db4 = self._parts28()
        bias = self.f28_bias
        dbd = bias.narrow(0, 0, B * 3136)
        db3 = bias.narrow(0, B * 3136, B * 32)
        db2 = bias.narrow(0, B * 3168, 2 * B * 64)  # [2][M][64] for a batch of M
        db1 = bias.narrow(0, B * 3296, B * 32)
        a1, a2, d0, d1 = self.acts["enc1"], self.acts["enc2"], self.acts["dec_fc"], self.acts["dec1"]
        gd1, gd0, ga2, ga1 = self.gacts["dec1"], self.gacts["dec_fc"], self.gacts["enc2"], self.gacts["enc1"]
        fwd = self._fwd_table28(X, idx, st.train_state, True, stamps=self.f28_stamps[0], prefetch=True)
        bwd = dict(self._f28_weight_table(), hparams=st.hparams, mulv=self.mulv, eps=self.eps, a1=a1, a2=a2, d0=d0,
                   d1=d1, dlog=self.dlog32, gd1=gd1, gd0=gd0, dbd_part=dbd, dmulv=self.dmulv, dmulv16=self.dmulv16,
                   ga2=ga2, ga1=ga1, db3_part=db3, db2_part=db2, db1_part=db1, stamps=self.f28_stamps[1])
        # the names are resolved and every tensor checked here, once: the step launches with these
        launch = dict(fwd=C.f28_table("forward", fwd, B, M), bwd=C.f28_table("backward", bwd, B, M),
                      pair=C.f28_table("pair", self._pair_table28(), B, M))
        # weight gradients: (G, X) per layer in the conv view (see _backward_hip)
        srcs = {"enc1": (ga1, self.xb), "enc2": (ga2, a1), "enc_head": (self.dmulv16, a2),
                "dec_fc": (gd0, self.z16), "dec1": (d0, gd1), "dec2": (d1, self.dlog32)}
        slabs, jobs = {}, []
        for name, (G, Xw) in srcs.items():
            l = self.by_name[name]
            d = self._desc(l, M)
            ns = wgrad_plan(d).nsplit
            t = torch.empty(ns * math.prod(_w_shape(l)), **f32)
            slabs[name + ".weight"] = (t, ns)
            jobs.append(self._job(lambda j: C.wgrad(G, Xw, d, t, job=j)))
        jobs.append(self._job(lambda j: C.loss_finalize2(bce, M, kld, M, st.train_state, st.hparams, True, job=j,
                                                         advance_step=True)))
        # bias gradients: per-sample partial rows written by the fused kernels
        for name, t, rows in (("enc1", db1, M), ("enc2", db2, 2 * M), ("enc_head", self.dmulv, M),
                              ("dec_fc", dbd, M), ("dec1", db3, M), ("dec2", db4, M)):
            slabs[name + ".bias"] = (t, rows)
        segs = self._seg_rows(slabs)
        units, layer_units = self._finalize_units(segs)
        pack, grid = C.pack_jobs_multi(jobs)
        # intra-group DDP: the decoder's weight gradients (ready first in the
        # reference's backward order) get a launch of their own, so their
        # bucket's all-reduce runs while the encoder's are still computed
        names = list(srcs)
        dec_jobs = [jobs[i] for i, n in enumerate(names) if n.startswith("dec")] + [jobs[len(names)]]
        enc_jobs = [jobs[i] for i, n in enumerate(names) if not n.startswith("dec")]
        dec_pack, dec_grid = C.pack_jobs_multi(dec_jobs)
        enc_pack, enc_grid = C.pack_jobs_multi(enc_jobs)
        first_dec = self.spec.index(self.dec[0])
        p = dict(fwd=fwd, bwd=bwd, launch=launch, jobs=jobs, jobs_pack=pack.to(dev), jobs_grid=grid, slabs=slabs,
                 segs=C.make_grad_segs(segs, dev.index or 0), units=C.make_grad_units(units, dev.index or 0),
                 nunits=len(units), layer_units=layer_units, first_dec=first_dec,
                 dec_pack=dec_pack.to(dev), dec_grid=dec_grid, enc_pack=enc_pack.to(dev), enc_grid=enc_grid,
                 dec_jobs=dec_jobs, enc_jobs=enc_jobs, names=names)
        p["epi_src"] = (M, srcs, segs, units)  # _epi_plan28, built on first use
        self._plans28[M] = p
        return p

    _EPI_ADAM28 = ("enc_head", "dec_fc")

    def _epi_plan28(self, p):
        """Second job table and finalize unit list of the fused 28x28 step
        (built on first use, then cached in the plan): the Linear layers'
        weight gradients as jobs that apply Adam in their epilogue, and the
        finalize without those two weight segments (their biases and every
        other layer stay). None when a layer's weight gradient runs more than
        one m-split at this M (its slabs then need the finalize's reduction)."""
        if "epi" not in p:
            p["epi"] = self._build_epi_plan28(p, *p["epi_src"])
        return p["epi"]

    def _build_epi_plan28(self, p, M, srcs, segs, units):
        C, dev = self.C, self.device
        seg_of = {l.name: 2 * i for i, l in enumerate(self.spec)}  # _seg_rows: weight, bias per layer
        for n in self._EPI_ADAM28:
            if p["slabs"][n + ".weight"][1] != 1 or segs[seg_of[n]][0] % 4 or segs[seg_of[n]][1] % 4:
                return None
        jobs = list(p["jobs"])
        for n in self._EPI_ADAM28:
            G, Xw = srcs[n]
            jobs[p["names"].index(n)] = self._job(lambda j: C.wgrad(
                G, Xw, self._desc(self.by_name[n], M), p["slabs"][n + ".weight"][0], job=j,
                adam=[self.params, self.exp_avg, self.exp_avg_sq, self.w16], adam_off=segs[seg_of[n]][0],
                adamc=self.f28_adamc))
        skip = {seg_of[n] for n in self._EPI_ADAM28}
        eunits = [u for u in units if u[0] not in skip]
        pack, grid = C.pack_jobs_multi(jobs)
        return dict(jobs=jobs, jobs_pack=pack.to(dev), jobs_grid=grid,
                    units=C.make_grad_units(eunits, dev.index or 0), nunits=len(eunits))

    def _step28(self, M):
        """Fused 28x28 step: forward + backward-data (one launch: f28_step_k,
        or two with MDT_F28_MERGE=0) || weight gradients + loss/step ||
        finalize + Adam (DDP: finalize without Adam, bucket all-reduce, then
        Adam + bf16 cast). Without a reducer the two Linear layers' weight
        gradients apply Adam themselves (MDT_F28_EPI_ADAM, _epi_plan28) and
        the finalize launch covers the rest."""
        C, p, st = self.C, self._plan28(M), self.state
        red = self.reducer
        # Adam in the Linear weight gradients' epilogues: chosen per call (tests
        # flip the switches between steps of one trainer). Only then does the
        # step kernel get the buffer to hand the step's Adam constants over in
        epi = (self._epi_plan28(p) if self.f28_epi_adam and red is None and self.f28_merge
               and not self.f28_skip_adam else None)
        t = p["launch"]
        if self.f28_merge:
            C.f28_step(t["fwd"], t["bwd"], self.B, M, self.rng_stream, pair=t["pair"] if self.f28_pair else {},
                       pair_delay_us=self.f28_pair_delay_us, **({"adamc": self.f28_adamc} if epi else {}))
        else:
            C.f28_forward(t["fwd"], self.B, M, self.rng_stream, True)
            C.f28_backward(t["bwd"], M, state=st.train_state)
        if red is None:
            q = epi or p
            C.launch_jobs_multi(q["jobs_pack"], q["jobs_grid"])
            self._grad_finalize(p["segs"], q["units"], 0, q["nunits"], not self.f28_skip_adam,
                                gather=([self._data[0], self._data[1], self.f28_xn, self.f28_xtag]
                                        if self.f28_prefetch else []), gather_B=self.B)
            return
        if self._comm_ctx():
            # fused xGMI all-reduce (comm_jobs.h), one stream: decoder weight
            # gradients | encoder weight gradients || decoder push (its bytes
            # cross the links while the encoder's are computed) | encoder
            # push+reduce || decoder reduce, both with Adam + bf16 cast.
            # MDT_DDP_OVERLAP=0: all weight gradients | push+reduce+Adam.
            packs = self._comm_packs28(M, p)
            for i, (pack, grid) in enumerate(packs):
                C.launch_jobs_multi(pack, grid)
                if self.comm_phase_hook is not None and i == len(packs) - 2:
                    self.comm_phase_hook()
            return
        # DDP (reference: the Reducer's bucket all-reduces launched from the
        # autograd hooks while backward continues, /root/reference/vae-hpo.py:72,
        # :130): decoder weight gradients -> their finalize -> every bucket
        # that holds only decoder parameters goes out on the comm stream ->
        # encoder weight gradients (overlapping those all-reduces) -> their
        # finalize -> the remaining buckets -> wait -> Adam + bf16 cast.
        lu, fd, L = p["layer_units"], p["first_dec"], len(self.spec)
        dec0 = self.layer_ranges()[fd][1]
        bounds = list(red.bounds())
        nbk = len(bounds) - 1
        early = self._overlap28(fused=False)
        if hasattr(red, "set_inline"):
            red.set_inline(not early)
        if not early:
            # one stream: all weight gradients | finalize | the bucket
            # collectives in issue order on the compute stream (no events) | Adam
            C.launch_jobs_multi(p["jobs_pack"], p["jobs_grid"])
            self._finalize_unit_range(p, lu[0], lu[L])
            for k in reversed(range(nbk)):
                red.launch(k)
        else:
            C.launch_jobs_multi(p["dec_pack"], p["dec_grid"])
            self._finalize_unit_range(p, lu[fd], lu[L])
            for k in reversed(range(nbk)):
                if bounds[k] >= dec0:
                    red.launch(k)
            C.launch_jobs_multi(p["enc_pack"], p["enc_grid"])
            self._finalize_unit_range(p, lu[0], lu[fd])
            for k in reversed(range(nbk)):
                if bounds[k] < dec0:
                    red.launch(k)
        red.wait_all()
        if not self.f28_skip_adam:
            self._adam_cast(True)

    def _comm_packs28(self, M, p):
        """Job tables of the fused-reducer 28x28 step after the f28_step_k
        launch: [(device pack, grid)], built once per (M, Adam, overlap)."""
        adam = not self.f28_skip_adam
        overlap = self._overlap28(fused=True) and not self.comm_split_tail
        key = (M, adam, overlap, self.comm_split_tail)
        packs = self._comm_packs.get(key)
        if packs is not None:
            return packs
        C, dev = self.C, self.device
        lu, fd, L = p["layer_units"], p["first_dec"], len(self.spec)
        segs, units = p["segs"], p["units"]
        jobs = p["jobs"]  # the weight-gradient jobs in p["names"] order + loss/step
        enc, dec = p["enc_jobs"], p["dec_jobs"]  # dec: with the loss/step job
        if self.comm_split_tail:
            tables = [jobs, [self._comm_job(segs, units, lu[0], lu[L], 1, adam)],
                      [self._comm_job(segs, units, lu[0], lu[L], 2, adam)]]
        elif overlap:
            tables = [dec,
                      enc + [self._comm_job(segs, units, lu[fd], lu[L], 1, adam)],
                      [self._comm_job(segs, units, lu[0], lu[fd], 3, adam),
                       self._comm_job(segs, units, lu[fd], lu[L], 2, adam)]]
        else:
            tables = [jobs, [self._comm_job(segs, units, lu[0], lu[L], 3, adam)]]
        self._comm_tables[key] = tables
        packs = []
        for i, t in enumerate(tables):
            st = self.comm_stamps[i] if self.comm_stamps is not None and i < len(self.comm_stamps) else None
            pack, grid = C.pack_jobs_multi(t, stamps=st)
            packs.append((pack.to(dev), grid))
        self._comm_packs[key] = packs
        return packs

    def _overlap28(self, fused: bool) -> bool:
        """Resolve MDT_DDP_OVERLAP (``ddp_overlap``; None = auto) for the fused
        28x28 DDP step: the split costs ~6 us with the fused xGMI jobs and
        ~31 us with RCCL on its own stream (profiles/r4_ddp_fused)."""
        if self.ddp_overlap is not None:
            return bool(self.ddp_overlap)
        from ..parallel.ddp import overlap_pays

        return overlap_pays(4 * (self.numel - self.split), 6.0 if fused else 31.0)

    def _finalize_unit_range(self, p, u0, u1):
        """Slab reduction into the gradient arena (no Adam) of finalize units [u0, u1)."""
        if u1 > u0:
            self._grad_finalize(p["segs"], p["units"], u0, u1, False)

    def _f28_weights(self):
        """(weight, bias) per layer in spec order; the single-channel edge layers read the f32 masters."""
        edge = (self.spec[0], self.spec[-1])
        return [t for l in self.spec for t in ((self._wf32 if l in edge else self._w)(l), self._b(l))]

    def _parts28(self):
        """f28_part as (bce, kld, dec2-bias partials)."""
        return [self.f28_part.narrow(0, i * self.B, self.B) for i in range(3)]

    def _f28_weight_table(self):
        """``_f28_weights`` under their slot names (``C.f28_slot_names()``)."""
        return dict(zip(self.C.f28_slot_names()["weights"], self._f28_weights()))

    def _fwd_table28(self, X, idx, state, acts, recon=None, stamps=None, prefetch=False):
        """The fused forward's tensors by slot name, every slot of the table a
        key (None = a null argument). ``state``: the train or the eval state;
        ``acts``: the activation outputs a backward reads (a launch with
        train = True needs them); ``recon``, ``stamps``: optional outputs;
        ``prefetch``: the rows the previous step's finalize gathered."""
        bce, kld, db4 = self._parts28()
        a1, a2, d0, d1 = ((self.acts[k] for k in ("enc1", "enc2", "dec_fc", "dec1")) if acts else (None,) * 4)
        return dict(self._f28_weight_table(), X=X, idx=idx, state=state, hparams=self.state.hparams, xb=self.xb,
                    a1=a1, a2=a2, mulv=self.mulv, eps=self.eps, z16=self.z16, d0=d0, d1=d1,
                    dlog=self.dlog32 if acts else None, recon=recon, bce_part=bce, kld_part=kld, db4_part=db4,
                    stamps=stamps, xn=self.f28_xn if prefetch else None, xtag=self.f28_xtag if prefetch else None)

    def _pair_table28(self):
        """The paired launches' exchange state by slot name."""
        return dict(xg=self.f28_xg, pairw=self.f28_pairw, err=self.f28_err)

    def _eval_fwd28(self, X, idx, want_recon):
        """Tensor table of the fused forward over an eval set: the eval state,
        no activation outputs (train = 0), the reconstruction when wanted."""
        return self._fwd_table28(X, idx, self.state.eval_state, False, recon=self.recon if want_recon else None)

    def _eval_batch28(self, M, X, idx, want_recon):
        # the fused 28x28 forward in eval mode (f28_fwd_k, one workgroup
        # per sample, no activation stores): one launch instead of the
        # layer path's dozen; its loss job advances the eval step exactly
        # like the layer path's step_begin (same Philox keys, same ring slot)
        st = self.state
        bce, kld, _ = self._parts28()
        # paired (two workgroups per sample, 2M CUs) unless MDT_F28_EVAL_PAIR=0
        pair = self._pair_table28() if self.f28_pair and self._eval_pair else {}
        self.C.f28_forward(self._eval_fwd28(X, idx, want_recon), self.B, M, EVAL_STREAM + self.rng_stream,
                           False, pair=pair)
        self.C.loss_finalize2(bce, M, kld, M, st.eval_state, st.hparams, True, advance_step=True)
