"""Layer-by-layer step engine of ``ConvVaeTrainer`` (a mixin over the trainer's
arenas, weight views and buffers, models/conv_vae.py): a GEMM per layer and
direction, independent launches fused horizontally (conv_jobs.hip). It trains
128x128 and z != 32 and serves the decode, IW and latent passes at every size."""

import math
import os
import sys

import torch

from ..ops.conv_plans import igemm_plan, wgrad_plan
from .conv_spec import _w_shape

TR_UNIT_WORDS = 16  # one TrUnit row (4 int32) of the uint8 ``tr_units`` table, in its elements


class LayerPathStep:
    def _n_bce(self, M):
        """Number of BCE loss partials the forward writes for a batch of M."""
        if self._thin_last:
            return self.C.thin_blocks(True, self._desc(self.spec[-1], M))
        return -(-M * self.D // 256)

    def _n_kld(self, M):
        """Number of KLD partials the forward writes for a batch of M (one per
        block of the reparameterisation kernel that ends the encoder)."""
        ks = igemm_plan(0, self._desc(self.enc[-1], M), True, fwd=True).ksplit
        if ks > 1:
            return self.C.combine_reparam_blocks(ks, M, self.Z)
        return -(-M * self.Z // 256)

    def _plan(self, M):
        """Per-batch-size backward plan: partial-slab buffers sized from the
        native planners, the GradSeg/GradUnit tables of the finalize kernel and
        the split-K workspace (built once per M, reused by every step/graph)."""
        p = self._plans.get(M)
        if p is not None:
            return p
        C, dev = self.C, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        slabs, colsum, ws_need, spec = {}, {}, 0, self.spec
        ws_words = lambda q: q.ksplit * q.m * q.ncols if q.ksplit > 1 else 0  # f32 split-K partials of a GEMM
        for i, l in enumerate(spec):
            d = self._desc(l, M)
            ns = wgrad_plan(d).nsplit
            wn = math.prod(_w_shape(l))
            if ns > 1:
                slabs[l.name + ".weight"] = (torch.empty(ns * wn, **f32), ns)
            # backward-data producing the previous layer's gradient
            if i == 0:
                continue
            prev = spec[i - 1]
            if i == len(spec) - 1 and self._thin_last:
                rows, ncols = C.thin_blocks(False, d), prev.cout
                colsum[prev.name] = t = torch.empty(rows * ncols, **f32)
                slabs[prev.name + ".bias"] = (t, rows)
                continue
            mode = 0 if l.kind == "convT" else 1
            split_ok = l.name == "dec_fc"
            q = igemm_plan(mode, d, split_ok)
            if split_ok:
                ws_need = max(ws_need, ws_words(q))
            if prev.name in ("dec_fc",) or l.name == "dec_fc":
                continue  # per-feature / reparam biases: colsum kernel below
            rows, ncols = q.colsum_rows, q.ncols
            colsum[prev.name] = t = torch.empty(rows * ncols, **f32)
            slabs[prev.name + ".bias"] = (t, rows * (ncols // prev.cout))
        for l in spec:  # forward split-K (deep, narrow conv-mode layers such as enc_head)
            if l.kind != "convT":
                ws_need = max(ws_need, ws_words(igemm_plan(0, self._desc(l, M), True, fwd=True)))
        # the layer feeding the encoder head, when it runs split-K: its combine
        # is folded into the head GEMM's A staging (APro, conv_igemm_dev.h)
        ws_a, ks_a = None, 0
        enc = self.enc
        if len(enc) >= 3 and os.getenv("MDT_CONV_APRO", "1") != "0":
            src = enc[-2]
            if not (src is spec[0] and self._thin_first) and src.kind == "conv" and src.cout % 8 == 0:
                q = igemm_plan(0, self._desc(src, M), True, fwd=True)
                if q.ksplit > 1:
                    ks_a, ws_a = q.ksplit, torch.empty(ws_words(q), **f32)
        rows_per = 8  # colsum kernel partial rows for the per-feature biases
        ncs = -(-M // rows_per)
        for l in (self.by_name["enc_head"], self.by_name["dec_fc"]):
            colsum[l.name] = t = torch.empty(ncs * l.cout, **f32)
            slabs[l.name + ".bias"] = (t, ncs)
        if self.channels != 1:
            raise NotImplementedError("conv-VAE HIP path: multi-channel images need the per-channel dlogits sum")
        nb = self._n_bce(M)
        gpart = torch.empty(nb, **f32)
        slabs[spec[-1].name + ".bias"] = (gpart, nb)
        segs = self._seg_rows(slabs)
        units, layer_units = self._finalize_units(segs)
        p = dict(slabs=slabs, colsum=colsum, gpart=gpart, ws=torch.empty(max(ws_need, 1), **f32), rows_per=rows_per,
                 ws_a=ws_a, ks_a=ks_a,
                 segs=C.make_grad_segs(segs, dev.index or 0), units=C.make_grad_units(units, dev.index or 0),
                 nunits=len(units), layer_units=layer_units)
        self._plans[M] = p
        return p

    def _layer_fwd(self, l, h, M, o16, o32, ws, **pro):
        """conv / linear: conv-mode GEMM; convT: parity-class GEMM on the
        transposed weights (no zero-insertion taps); single-channel edge
        layers: direct kernels."""
        d = self._desc(l, M)
        if l is self.spec[0] and self._thin_first:
            self.C.thin_conv(h, self._wf32(l), d, self._b(l), l.relu, o16)
        elif l is self.spec[-1] and self._thin_last:
            self.C.thin_tconv(h, self._wf32(l), d, self._b(l), y32=o32)
        elif l.kind == "convT":
            self.C.igemm(1, h, self._wt(l), d, self._b(l), l.relu, o16, o32, fwd=True)
        else:
            self.C.igemm(0, h, self._w(l), d, self._b(l), l.relu, o16, o32, ws=ws, fwd=True, **pro)

    def _forward_hip(self, M, state, stream, want_recon=False, train=True, src=None, enc_only=False):
        """Forward of one batch. ``src = (X, idx)``: the batch is gathered from
        the dataset by the step's first kernel (and the step begun there) when
        the first layer runs on the direct kernel; otherwise by gather_rows.
        ``enc_only``: stop once ``self.mulv`` is written (the importance-weighted
        pass draws its own samples and runs the decoder per chunk)."""
        C, p, hp = self.C, self._plan(M), self.state.hparams
        enc, dec = self.enc, self.dec
        h, first = self.xb, 0
        # w16t of the previous step's update still to be written (an eval
        # forward finds them current: evaluate() ran _ensure_wt first)
        wt = self._wt_deferred() and train
        if src is not None:
            X, idx = src
            l = enc[0]
            if self.fuse_jobs and self._thin_first and len(enc) > 1:
                first_conv = (lambda job, l=l: C.thin_conv(X, self._wf32(l), self._desc(l, M), self._b(l), l.relu,
                                                           self.acts[l.name], job=job, idx=idx, state=state,
                                                           hparams=hp, B=self.B, xb=self.xb))
                if wt and not self.wt_in_dec:
                    # the transposed copies share the step's first launch (nothing in it reads them)
                    self._run_group([first_conv, lambda job: self._wtrans_layers(1, len(self.spec), job)])
                    wt = False
                else:
                    first_conv(None)
                h, first = self.acts[l.name], 1
            else:
                C.step_begin(state, hp)
                C.gather_rows(X, idx, state, self.B, M, self.xb)
        if wt and not (self.wt_in_dec and self.fuse_jobs):
            self._wtrans_layers(1, len(self.spec))
            wt = False
        pro = {}
        for l in enc[first:]:
            last = l is enc[-1]
            if not last and p["ws_a"] is not None and l is enc[-2]:
                # split-K partials only; the head's A staging combines them (+bias, ReLU)
                # and writes this layer's activations for the backward
                C.igemm(0, h, self._w(l), self._desc(l, M), None, False, None, None, ws=p["ws_a"], combine=False,
                        fwd=True)
                pro = dict(a_slab=p["ws_a"], a_ks=p["ks_a"], a_bias=self._b(l), a_relu=l.relu,
                           a_out16=self.acts[l.name])
                h = self.acts[l.name]
                continue
            if last:
                ks = igemm_plan(0, self._desc(l, M), True, fwd=True).ksplit
                if ks > 1:  # split-K head: combine fused with the reparameterisation
                    C.igemm(0, h, self._w(l), self._desc(l, M), self._b(l), False, None, self.mulv, ws=p["ws"],
                            combine=False, fwd=True, **pro)
                    C.combine_reparam(p["ws"], ks, self._b(l), self.mulv, self.eps, self.z16, None, M, self.Z,
                                      state, hp, stream, self.kld_part)
                    if enc_only:
                        return
                    self._tc_forward(M, train)
                    break
            self._layer_fwd(l, h, M, None if last else self.acts[l.name], self.mulv if last else None, p["ws"],
                            **(pro if last else {}))
            h = self.acts[l.name]
        else:
            if enc_only:
                return
            C.reparam(self.mulv, self.eps, self.z16, None, M, self.Z, state, hp, stream, self.kld_part)
            self._tc_forward(M, train)
        h = self.z16
        for l in dec:
            last = l is dec[-1]
            if wt:
                # the transposed copies share the first decoder launch: nothing
                # before it reads them, the parity-mode layers after it do
                wt = False
                d = self._desc(l, M)
                if (l.kind != "convT" and not last and igemm_plan(0, d, p["ws"] is not None).ksplit == 1):
                    self._run_group([lambda job, l=l, d=d, h=h: C.igemm(0, h, self._w(l), d, self._b(l), l.relu,
                                                                        self.acts[l.name], None, job=job),
                                     lambda job: self._wtrans_layers(1, len(self.spec), job)])
                    h = self.acts[l.name]
                    continue
                self._wtrans_layers(1, len(self.spec))
            if last and self._thin_last:  # last layer + BCE + dlogits + bias-grad partials, one launch
                C.thin_tconv(h, self._wf32(l), self._desc(l, M), self._b(l), X=self.xb,
                             dlog16=self.dlog16 if train else None, recon=self.recon if want_recon else None,
                             part=self.bce_part, gpart=p["gpart"] if train else None)
                return
            self._layer_fwd(l, h, M, None if last else self.acts[l.name], self.logits if last else None, p["ws"])
            h = self.acts[l.name]
        C.bce_logits(self.logits, self.xb, None, M, self.D, self.dlog16 if train else None,
                     self.recon if want_recon else None, self.bce_part, p["gpart"] if train else None)

    def _tc_forward(self, M, training_step):
        """Training step with the total-correlation penalty: its forward and
        backward kernels (vae_tc.hip), which need only the step's mulv and eps;
        the fold runs after the reparameterisation backward (``_backward_hip``)."""
        if self.tc_on and training_step:
            self.C.tc_penalty(self.mulv, self.eps, M, self.Z, self.tc_ws, self.tc_value,
                              state=self.state.train_state, stage=1)

    # ----------------------------------------------------------- job fusion
    def _launch_fused(self, jobs, what) -> bool:
        """Issue recorded ``jobs`` as ONE fused kernel when conv_jobs.hip has an
        instantiation for their kinds; False (nothing launched) when not."""
        if all(j.kind > 0 for j in jobs) and self.C.launch_jobs(jobs):
            self._fused_launches += 1
            return True
        if os.getenv("MDT_JOBS_DEBUG"):
            print(f"[jobs] {what}: kinds={sorted(j.kind for j in jobs)} post={[j.has_post for j in jobs]}",
                  file=sys.stderr, flush=True)
        return False

    def _run_group(self, fns):
        """Run independent launches ``fns`` (each ``f(job)``): recorded as jobs
        and issued as ONE fused kernel when conv_jobs.hip has an instantiation
        for their kinds, else each op's own kernel (same bodies, same results)."""
        if self.fuse_jobs and 1 < len(fns) <= 3 and \
                self._launch_fused([self._job(f) for f in fns], "not fused"):
            return
        for f in fns:
            f(None)

    def _backward_hip(self, M, with_loss=False, optimizer=False):
        """Reverse sweep: per layer one weight-gradient GEMM (partial slabs) and
        one backward-data GEMM whose epilogue applies the previous layer's ReLU
        mask and emits its bias-gradient column sums. The two (plus any bias
        column sum or loss reduction that became ready) are independent and
        share one launch (``_run_group``). ``with_loss`` adds the loss reduction
        of the forward to the first launch; ``optimizer`` (no reducer) appends
        the optimizer tail: first-layer weight gradient || finalize+Adam of the
        other layers, then first-layer finalize || transposed weight copies."""
        C, p, spec, st = self.C, self._plan(M), self.spec, self.state
        g, red = self.dlog16, self.reducer
        # fused xGMI all-reduce (comm_jobs.h): a backward launch with a free job
        # slot also pushes the layers the previous launches completed
        # (``pending``); the tail pushes the rest, reduces and applies Adam
        fused = red is not None and self.fuse_jobs and bool(self._comm_ctx())
        pend_lo = pend_hi = len(spec)  # layers [pend_lo, pend_hi) complete, not yet pushed
        if fused:
            red = None
        if red is not None:
            bounds = list(red.bounds())
            starts = {b: i for i, (l, b, e) in enumerate(self.layer_ranges())}
            assert all(b in starts or b == self.numel for b in bounds), "bucket bounds must fall on layer starts"
        carry = []  # launches that depend on the previous group's outputs
        # spread mode: layers [fin_hi, L) already finalized (+Adam) as the third
        # job of a backward launch -- layer j's gradients are complete once the
        # launch of layer j ran, and nothing later in the step reads its weights
        spread = (optimizer and self.spread_fin and self.fuse_jobs and self.reducer is None)
        fin_hi = len(spec)
        if with_loss:
            carry.append(lambda job: C.loss_finalize2(self.bce_part, self._n_bce(M), self.kld_part,
                                                      self._n_kld(M), st.train_state, st.hparams, True,
                                                      job=job))
        for i in range(len(spec) - 1, -1, -1):
            if red is not None and i + 1 < len(spec):
                self._maybe_launch_bucket(red, bounds, starts, i + 1, M)
            l = spec[i]
            prev = spec[i - 1] if i > 0 else None
            d = self._desc(l, M)
            if i == 0:
                a_in = self.xb
            elif l.name == "dec_fc":
                a_in = self.z16
            else:
                a_in = self.acts[prev.name]
            wslab = p["slabs"].get(l.name + ".weight")
            wout = wslab[0] if wslab is not None else self._gw(l)
            fns, carry, after = carry, [], []
            if l.kind == "convT":  # conv view: output = convT input, input = convT output
                fns.append(lambda job, a_in=a_in, g=g, d=d, wout=wout: C.wgrad(a_in, g, d, wout, job=job))
            else:
                fns.append(lambda job, a_in=a_in, g=g, d=d, wout=wout: C.wgrad(g, a_in, d, wout, job=job))
            gin = None
            if prev is not None:
                omask = a_in if prev.relu else None
                if l.name == "dec_fc":
                    ks = igemm_plan(1, d, True).ksplit
                    fns.append(lambda job, g=g, l=l, d=d, ks=ks: C.igemm(1, g, self._wt(l), d, None, False, None,
                                                                         self.dz, ws=p["ws"], job=job,
                                                                         combine=ks == 1))
                    if ks > 1:  # split-K combine fused with the reparameterisation backward
                        after.append(lambda ks=ks: C.combine_reparam_bwd(p["ws"], ks, self.mulv, self.eps, self.dmulv,
                                                                         self.dmulv16, self.dz, M, self.Z,
                                                                         st.hparams, state=st.train_state))
                    else:
                        after.append(lambda: C.reparam_bwd(self.dz, self.mulv, self.eps, self.dmulv, self.dmulv16,
                                                           M, self.Z, st.hparams, state=st.train_state))
                    if self.tc_on:
                        # the penalty's share, added in place to d[mu|lv] (bf16 copy rewritten) by the fold
                        # kernel of vae_tc.hip; its forward and backward ran after the reparameterisation
                        after.append(lambda: C.tc_penalty(self.mulv, self.eps, M, self.Z, self.tc_ws, self.tc_value,
                                                          state=st.train_state, dmulv=self.dmulv,
                                                          dmulv16=self.dmulv16, stage=2))
                    cso = p["colsum"][prev.name]
                    carry.append(lambda job, cso=cso: C.colsum(self.dmulv16, M, 2 * self.Z, p["rows_per"], cso,
                                                               job=job))
                    gin = self.dmulv16
                elif i == len(spec) - 1 and self._thin_last:
                    gin = self.gacts[prev.name]
                    cso = p["colsum"][prev.name]
                    fns.append(lambda job, g=g, l=l, d=d, gin=gin, omask=omask, cso=cso:
                               C.thin_conv(g, self._wf32(l), d, None, False, gin, omask, cso, job=job))
                else:
                    gin = self.gacts[prev.name]
                    cs = None if prev.name == "dec_fc" else p["colsum"].get(prev.name)
                    mode = 0 if l.kind == "convT" else 1
                    w = self._w(l) if l.kind == "convT" else self._wt(l)
                    fns.append(lambda job, g=g, w=w, d=d, gin=gin, omask=omask, cs=cs, mode=mode:
                               C.igemm(mode, g, w, d, None, False, gin, None, omask, cs, job=job))
                    if prev.name == "dec_fc":
                        cso = p["colsum"][prev.name]
                        carry.append(lambda job, gin=gin, n=prev.cout, cso=cso:
                                     C.colsum(gin, M, n, p["rows_per"], cso, job=job))
            if prev is None and optimizer:
                if fin_hi > 1:
                    fns.append(lambda job, hi=fin_hi: self._finalize_layers(M, 1, hi, job))
                self._run_group(fns)
                if self._wt_deferred():
                    self._finalize_layers(M, 0, 1)
                else:
                    self._run_group([lambda job: self._finalize_layers(M, 0, 1, job),
                                     lambda job: self._wtrans_layers(1, len(spec), job)])
                break
            if spread and len(fns) == 2 and i + 1 < fin_hi and self._run_with_finalize(fns, M, i + 1, fin_hi):
                fin_hi = i + 1
            elif fused and len(fns) in (1, 2) and pend_lo < pend_hi and \
                    self._run_with_comm(fns, M, pend_lo, pend_hi):
                pend_hi = pend_lo
            else:
                self._run_group(fns)
            for f in after:
                f()
            if fused:
                pend_lo = i  # layer i's gradients are complete now
            if prev is None:
                assert not carry
                if red is not None:
                    self._maybe_launch_bucket(red, bounds, starts, 0, M)
                if fused:
                    self._comm_tail(M, pend_lo, pend_hi)
                break
            g = gin

    def _run_with_finalize(self, fns, M, lo, hi):
        """Launch the two jobs ``fns`` plus finalize+Adam of layers [lo, hi) as
        ONE kernel; False (nothing launched) when that combination has no
        instantiation."""
        fin = lambda job: self._finalize_layers(M, lo, hi, job)
        return self._launch_fused([self._job(f) for f in fns + [fin]], "no finalize fusion")

    def _run_with_comm(self, fns, M, lo, hi):
        """Launch the jobs ``fns`` plus the push (comm_jobs.h, mode 1) of layers
        [lo, hi) as ONE kernel; False (nothing launched) when that combination
        has no instantiation."""
        p = self._plan(M)
        lu = p["layer_units"]
        push = lambda job: self._comm_job(p["segs"], p["units"], lu[lo], lu[hi], 1, not self.comm_skip_adam, job=job)
        return self._launch_fused([self._job(f) for f in fns + [push]], "no comm fusion")

    def _comm_tail(self, M, lo, hi):
        """After the first layer's backward launch: push+reduce+Adam of the
        layers not pushed yet ([lo, hi), the first layer included) || reduce+Adam
        of the ones pushed by the backward launches ([hi, L)), one launch."""
        p, L = self._plan(M), len(self.spec)
        lu, adam = p["layer_units"], not self.comm_skip_adam
        jobs = [self._comm_job(p["segs"], p["units"], lu[lo], lu[hi], 3, adam)]
        if hi < L:
            jobs.append(self._comm_job(p["segs"], p["units"], lu[hi], lu[L], 2, adam))
        if len(jobs) == 2:
            ok = self._launch_fused(jobs, "no comm tail")
            assert ok, "jobs_k<JComm, JComm> missing from conv_jobs.hip"
        else:
            pack, grid = self._comm_single_pack(("tail", M, lo, hi, adam), jobs[0])
            self.C.launch_jobs_multi(pack, grid)

    def _comm_single_pack(self, key, job):
        """Device job table of a single comm job (cached by ``key``: replayed
        graphs keep reading it)."""
        if key not in self._comm_packs:
            pack, grid = self.C.pack_jobs_multi([job])
            self._comm_packs[key] = (pack.to(self.device), grid)
        return self._comm_packs[key]

    def _wt_deferred(self):
        """The transposed weight copies (w16t) of a step's update are written by
        the next step's first launch or the first decoder launch (MDT_CONV_DEFER_WT)."""
        return self.defer_wt and self.fuse_jobs and self._thin_first and self.reducer is None and len(self.spec) > 1

    def _finalize_layers(self, M, lo, hi, job=None):
        """Finalize + Adam + bf16 cast of layers [lo, hi) (their units of the plan)."""
        p = self._plan(M)
        self._grad_finalize(p["segs"], p["units"], p["layer_units"][lo], p["layer_units"][hi], True, job=job)

    def _finalize_grads(self, M, do_adam):
        """Reduce the partial slabs into the gradient arena (deterministic order);
        with ``do_adam`` also apply Adam and re-emit the bf16 weight copies."""
        p = self._plan(M)
        self._grad_finalize(p["segs"], p["units"], 0, p["nunits"], do_adam)

    def _wtrans_layers(self, lo, hi, job=None):
        """Parity-ordered transposed copies of layers [lo, hi) (the first layer's
        copy is never read: it has no backward-data GEMM)."""
        t0, t1 = self._tr_layer[lo], self._tr_layer[hi]
        self.C.wtrans(self.w16, self.w16t, self.segs,
                      self.tr_units.narrow(0, t0 * TR_UNIT_WORDS, (t1 - t0) * TR_UNIT_WORDS), t1 - t0, job=job)

    def _maybe_launch_bucket(self, red, bounds, starts, i, M):
        """Layer i's gradients just became final (all layers >= i are done): if
        i starts a bucket, reduce that bucket's partial slabs into the arena and
        launch its all-reduce (it overlaps the rest of the backward)."""
        _, b, _ = self.layer_ranges()[i]
        if b not in bounds[:-1]:
            return
        k = bounds.index(b)
        end = bounds[k + 1]
        last = next((j for j, (l, bb, e) in enumerate(self.layer_ranges()) if bb >= end), len(self.spec))
        p = self._plan(M)
        self._grad_finalize(p["segs"], p["units"], p["layer_units"][i], p["layer_units"][last], False)
        red.launch(k)

    def _step_layers(self, M):
        self._forward_hip(M, self.state.train_state, self.rng_stream, src=self._data[:2])
        if self.reducer is None:
            # backward + optimizer tail (finalize/Adam/bf16 cast/transposes) in fused launches
            self._backward_hip(M, with_loss=True, optimizer=True)
            return
        # intra-group DDP: the backward finalizes + launches each gradient bucket
        # as it completes (loss reduction in its first launch); Adam after the
        # all-reduces. Fused xGMI reducer: pushes ride in the backward launches,
        # the tail reduces + applies Adam (no stream-side collectives to wait for)
        self._backward_hip(M, with_loss=True)
        if self.fuse_jobs and self._comm_ctx():
            self._wtrans_layers(1, len(self.spec))  # the first layer's copy is never read
            return
        self.reducer.wait_all()
        self._adam_cast(True)
        self._transpose_weights()

    def _decode_z16(self, V):
        """The decoder layers over rows ``z16[:V]`` into ``logits``."""
        dec = self.dec
        h, ws = self.z16, self._plan(V)["ws"]
        for l in dec:
            last = l is dec[-1]
            self._layer_fwd(l, h, V, None if last else self.acts[l.name], self.logits if last else None, ws)
            h = self.acts[l.name]
