"""Graph-replayed evaluation passes for the HIP trainers.

Reference: ``test()`` runs the model over the whole 10 000-image test set
after every epoch (/root/reference/vae-hpo.py:95-119), and its time is part of
the per-trial wall time the aggregate samples/s metric divides by
(:159, :172-174). Issued eagerly from Python, each test
batch costs a dozen kernel launches plus their host overhead: ~230 us per
batch, 17-19 ms per epoch for the 28x28 conv-VAE -- 37 % of an epoch whose
training takes 29 ms (`profiles/r5_e2e`).

The trainers' eval kernels take the batch rows from a device-resident cursor
(the eval ``TrainState``) and write the loss into its ring, exactly like the
training step, so a whole pass is capturable: batch 0 runs eagerly (it may
also produce the reconstruction images), the remaining full batches replay one
captured graph of S batches, the tail batch a graph of its own. The index list
lives in a persistent buffer (its address is baked into the graphs; each pass
copies the caller's indices into it), graphs are keyed by (S, M, dataset
address and length, buffer address; only the latest dataset's are kept), and
capturing restores the eval state
the warm-up batch advanced. Numerics are those of the eager pass (same kernels
in the same order).
"""

from __future__ import annotations

import numpy as np
import torch

from ..ops import native
from .iw import check_iw_args, default_chunk, iw_eps, iw_reduce
from .latent import check_latent_args, latent_eps, latent_report
from .sample_report import (COLS, bandwidths_of, check_sample_args, mean_pair_d2, sample_rows, sample_stats,
                            sample_z)

__all__ = ["GraphedEval", "GraphedIwEval", "GraphedLatentEval", "SampleEval", "capture_replayable"]


def capture_replayable(snapshot_tensors, launch, repeats: int):
    """A graph of ``repeats`` calls of ``launch()`` that leaves the device
    state as it found it: the warm-up call (plans, workspaces, communicators
    and code objects exist before capture) and the capture itself advance the
    step counter / cursor / Adam moments, so ``snapshot_tensors`` are cloned
    first and restored afterwards. The graph is uploaded before it is returned."""
    snap = [t.clone() for t in snapshot_tensors]
    cur = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        launch()
    cur.wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(repeats):
            launch()
    for t, v in zip(snapshot_tensors, snap):
        t.copy_(v)
    native.upload_graph(g)
    return g


class GraphedEval:
    """Mixin: requires ``self.B``, ``self.device``, ``self.use_graphs``,
    ``self.set_cursor``, ``self.reset_loss``, ``self._eval_batch(M, X, idx,
    want_recon)``, ``self._eval_state()`` (the eval TrainState tensor) and
    ``self._eval_recon(M)`` (the first batch's reconstruction)."""

    _eval_idx = None
    _eval_graphs = None

    def _eval_bind(self, idx_padded: torch.Tensor) -> torch.Tensor:
        n = idx_padded.numel()
        buf = self._eval_idx
        if buf is None or buf.numel() != n:
            self._eval_idx = buf = torch.empty(n, dtype=torch.int32, device=self.device)
            self._eval_graphs = {}
        buf.copy_(idx_padded)
        return buf

    def _eval_graph(self, S: int, M: int, X: torch.Tensor, idx: torch.Tensor):
        key = (S, M, X.data_ptr(), X.shape[0], idx.data_ptr())
        # graphs of the latest eval set only: a caller that passes
        # a new (e.g. temporary) X drops the graphs -- and their private memory
        # pools -- captured for the previous one instead of accumulating them
        xkey = (X.data_ptr(), X.shape[0], idx.data_ptr())
        if getattr(self, "_eval_xkey", None) != xkey:
            self._eval_graphs = {}
            self._eval_xkey = xkey
        g = self._eval_graphs.get(key)
        if g is None:
            g = capture_replayable([self._eval_state()], lambda: self._eval_batch(M, X, idx, False), S)
            self._eval_graphs[key] = g
        return g

    def _eval_graphed(self, X: torch.Tensor, idx_padded: torch.Tensor, n: int, want_first_recon: bool):
        """One eval pass over rows idx[:n] of X (graphs after batch 0)."""
        B = self.B
        nb = -(-n // B)
        idx = self._eval_bind(idx_padded)
        self.set_cursor(0, nb, eval=True)
        self.reset_loss(eval=True)
        M0 = min(B, n)
        self._eval_batch(M0, X, idx, want_first_recon)
        first = self._eval_recon(M0) if want_first_recon else None
        full, tail = n // B, n % B
        if n > B:
            if full > 1:
                self._eval_graph(full - 1, B, X, idx).replay()
            if tail:
                self._eval_graph(1, tail, X, idx).replay()
        return first


class GraphedIwEval:
    """Mixin: ``evaluate_iw``, the importance-weighted log-likelihood pass
    (models/iw.py), eager or graph-replayed like ``GraphedEval``'s passes and
    independent of them (own index buffer, own graphs, own device state).

    Requires ``self.B``, ``self.Z``, ``self.seed``, ``self.device``,
    ``self.backend``, ``self.use_graphs`` and

    * torch backend: ``self._iw_logw_torch(x, eps) -> logw[K, M]``;
    * hip backend: ``self._iw_prepare()`` (once per pass, before any launch),
      ``self._iw_begin(nbatches)`` (zero the pass state),
      ``self._iw_batch(M, X, idx, k, S, rows)`` (launch one batch at the pass
      cursor; ``rows`` is the float32 [2, nbatches*B] per-row result buffer),
      ``self._iw_state()`` (the pass's device state tensor),
      ``self._iw_read() -> (nll, neg_elbo)`` and ``self._iw_ws_token()`` (a
      value that changes whenever a workspace the launches use is reallocated).
    """

    _iw_idx = None
    _iw_rows = None
    _iw_graphs = None
    _iw_xkey = None

    def _iw_bind(self, idx_padded: torch.Tensor):
        n = idx_padded.numel()
        buf = self._iw_idx
        if buf is None or buf.numel() != n:
            self._iw_idx = buf = torch.empty(n, dtype=torch.int32, device=self.device)
            self._iw_rows = torch.zeros(2, n, dtype=torch.float32, device=self.device)
            self._iw_graphs = {}
        buf.copy_(idx_padded)
        return buf, self._iw_rows

    def _iw_graph(self, nbat: int, M: int, k: int, S: int, X: torch.Tensor, idx: torch.Tensor, rows: torch.Tensor):
        # batch 0 of this pass already ran eagerly at this (k, S): the workspaces have their final size
        xkey = (X.data_ptr(), X.shape[0], idx.data_ptr(), rows.data_ptr(), self._iw_ws_token())
        if self._iw_xkey != xkey:  # graphs of the latest eval set (and workspace) only, as GraphedEval
            self._iw_graphs = {}
            self._iw_xkey = xkey
        key = (nbat, M, k, S)
        g = self._iw_graphs.get(key)
        if g is None:
            g = capture_replayable([self._iw_state()], lambda: self._iw_batch(M, X, idx, k, S, rows), nbat)
            self._iw_graphs[key] = g
        return g

    @torch.no_grad()
    def evaluate_iw(self, X: torch.Tensor, idx: torch.Tensor, k: int, chunk_samples=None, return_rows: bool = False):
        """K-sample importance-weighted bound on -log p(x) and the K-sample
        negative ELBO (beta = 1) over rows ``X[idx]``, from the same draws.

        Returns ``dict(nll, neg_elbo, rows, k)`` (sums over the rows; with
        ``return_rows`` also float32 ``row_nll[n]`` / ``row_neg_elbo[n]``).
        The samples run in chunks of ``chunk_samples`` (default: as many as
        keep chunk x batch within 8192 decoder rows). Training and eval state
        are not touched; the result does not depend on ``rng_stream``."""
        check_iw_args(k, self.B, self.Z)
        k = int(k)
        S = default_chunk(k, self.B, chunk_samples)
        B = self.B
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        n = idx.numel()
        if n == 0:
            raise ValueError("evaluate_iw needs at least one row")
        nb = -(-n // B)
        X = X.contiguous()
        if self.backend != "hip":
            rn, re = [], []
            for b in range(nb):
                M = min(B, n - b * B)
                x = X[idx[b * B: b * B + M].long()]
                eps = torch.from_numpy(np.ascontiguousarray(iw_eps(k, B, self.Z, self.seed, b)[:, :M])).to(self.device)
                logw = torch.cat([self._iw_logw_torch(x, eps[s: s + S]) for s in range(0, k, S)], 0)
                a, e = iw_reduce(logw)
                rn.append(a.float())
                re.append(e.float())
            row_nll, row_ne = torch.cat(rn), torch.cat(re)
            nll, ne = float(row_nll.double().sum()), float(row_ne.double().sum())
        else:
            pad = nb * B - n
            if pad:
                idx = torch.cat([idx, idx[:1].expand(pad)])  # never read (rows >= M)
            self._iw_prepare()
            ibuf, rows = self._iw_bind(idx)
            self._iw_begin(nb)
            if self.use_graphs:
                self._iw_batch(min(B, n), X, ibuf, k, S, rows)
                full, tail = n // B, n % B
                if n > B:
                    if full > 1:
                        self._iw_graph(full - 1, B, k, S, X, ibuf, rows).replay()
                    if tail:
                        self._iw_graph(1, tail, k, S, X, ibuf, rows).replay()
            else:
                for b in range(nb):
                    self._iw_batch(min(B, n - b * B), X, ibuf, k, S, rows)
            nll, ne = self._iw_read()
            row_nll, row_ne = rows[0, :n], rows[1, :n]
        out = dict(nll=float(nll), neg_elbo=float(ne), rows=n, k=k)
        if return_rows:
            out["row_nll"], out["row_neg_elbo"] = row_nll.clone(), row_ne.clone()
        return out


class GraphedLatentEval:
    """Mixin: ``evaluate_latent``, the latent report (models/latent.py): active
    units and the MI / TC / dimension-wise-KL split of the KL term over rows
    ``X[idx]``. A pass of its own like ``GraphedIwEval``'s (own index buffer,
    own graphs, own device state): per batch the encoder and a collect kernel
    that files the batch's ``mu | lv`` rows into the pass buffer; after the last
    batch the once-per-pass kernels (csrc/kernels/vae_latent.hip) run eagerly.

    Requires ``self.B``, ``self.Z``, ``self.seed``, ``self.device``,
    ``self.backend``, ``self.use_graphs`` and

    * torch backend: ``self._lat_encode_torch(x) -> (mu, lv)``;
    * hip backend: ``self._lat_prepare()`` (once per pass, before any launch),
      ``self._lat_begin(nbatches)`` (zero the pass state),
      ``self._lat_batch(M, X, idx, rows)`` (launch one batch at the pass
      cursor; ``rows`` is the float32 [nbatches*B, 2Z] pass buffer),
      ``self._lat_state()`` (the pass's device state tensor) and
      ``self._lat_hparams()`` (the device HParams image: the Philox key).
    """

    # pairs per torch-backend block: [chunk, n, Z] float32 stays within 64 MiB
    LATENT_CHUNK_ELEMS = 1 << 24

    _lat_idx = None
    _lat_rows = None
    _lat_graphs = None
    _lat_xkey = None
    _lat_ws = None
    _lat_last = None

    def _lat_bind(self, idx_padded: torch.Tensor):
        n = idx_padded.numel()
        buf = self._lat_idx
        if buf is None or buf.numel() != n:
            self._lat_idx = buf = torch.empty(n, dtype=torch.int32, device=self.device)
            self._lat_rows = torch.zeros(n, 2 * self.Z, dtype=torch.float32, device=self.device)
            self._lat_graphs = {}
        buf.copy_(idx_padded)
        return buf, self._lat_rows

    def _lat_graph(self, nbat: int, M: int, X: torch.Tensor, idx: torch.Tensor, rows: torch.Tensor):
        xkey = (X.data_ptr(), X.shape[0], idx.data_ptr(), rows.data_ptr())
        if self._lat_xkey != xkey:  # graphs of the latest eval set only, as GraphedEval
            self._lat_graphs = {}
            self._lat_xkey = xkey
        key = (nbat, M)
        g = self._lat_graphs.get(key)
        if g is None:
            g = capture_replayable([self._lat_state()], lambda: self._lat_batch(M, X, idx, rows), nbat)
            self._lat_graphs[key] = g
        return g

    def _lat_workspaces(self, n: int):
        C = native.require()
        if self._lat_ws is None or self._lat_ws[0] != n:
            nf, nd = C.latent_ws_numel(n, self.Z)
            self._lat_ws = (n, [torch.zeros(nf, dtype=torch.float32, device=self.device),
                                torch.zeros(nd, dtype=torch.float64, device=self.device)])
        return self._lat_ws[1]

    @torch.no_grad()
    def evaluate_latent(self, X: torch.Tensor, idx: torch.Tensor, au_threshold: float = 0.01,
                        return_rows: bool = False) -> dict:
        """The latent report over rows ``X[idx]``: ``dict(rows, kl, kl_per_dim,
        mu_var, post_var, active_units, au_threshold, mi, tc, dwkl,
        sampled_kl)``, per-row means in nats, the per-dimension entries float32
        ``[Z]`` tensors; with ``return_rows`` also ``lq_joint``, ``lq_marg``,
        ``lq_cond``, ``lp`` ``[n]``. Training, eval and iw state are not
        touched; the result depends on (weights, data, seed, n) only."""
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        n = idx.numel()
        check_latent_args(n, self.Z, au_threshold)
        B, Z = self.B, self.Z
        nb = -(-n // B)
        X = X.contiguous()
        if self.backend != "hip":
            mulv = torch.cat([torch.cat(self._lat_encode_torch(X[idx[b * B: b * B + B].long()]), 1)
                              for b in range(nb)]).float()
            mu, lv = mulv[:, :Z], mulv[:, Z:]
            eps = torch.from_numpy(latent_eps(n, Z, self.seed)).to(self.device)
            out = latent_report(mu, lv, eps, au_threshold, chunk=max(1, self.LATENT_CHUNK_ELEMS // (n * Z)),
                                return_rows=return_rows)
            self._lat_last = dict(mulv=mulv.clone(), eps=eps, z=mu + eps * torch.exp(0.5 * lv))
            return out
        C = native.require()
        pad = nb * B - n
        if pad:
            idx = torch.cat([idx, idx[:1].expand(pad)])  # never read (rows >= M)
        self._lat_prepare()
        ibuf, rows = self._lat_bind(idx)
        self._lat_begin(nb)
        if self.use_graphs:
            self._lat_batch(min(B, n), X, ibuf, rows)
            full, tail = n // B, n % B
            if n > B:
                if full > 1:
                    self._lat_graph(full - 1, B, X, ibuf, rows).replay()
                if tail:
                    self._lat_graph(1, tail, X, ibuf, rows).replay()
        else:
            for b in range(nb):
                self._lat_batch(min(B, n - b * B), X, ibuf, rows)
        ws = self._lat_workspaces(n)
        st = self._lat_state()
        C.latent_report(rows, n, Z, st, self._lat_hparams(), ws)
        r = C.latent_state_read(st)
        view = lambda name: C.latent_ws_view(ws[0], n, Z, None, name).clone()
        mu_var = view("mu_var")
        out = dict(rows=n, kl=float(r[0]), kl_per_dim=view("kl_per_dim"), mu_var=mu_var, post_var=view("post_var"),
                   active_units=int((mu_var > au_threshold).sum()), au_threshold=float(au_threshold),
                   mi=float(r[1]), tc=float(r[2]), dwkl=float(r[3]), sampled_kl=float(r[4]))
        if return_rows:
            for k in ("lq_joint", "lq_marg", "lq_cond", "lp"):
                out[k] = view(k)
        self._lat_last = n
        return out

    def latent_buffers(self) -> dict:
        """``mulv[n, 2Z]``, ``eps[n, Z]`` and ``z[n, Z]`` of the last
        ``evaluate_latent`` pass (copies)."""
        last = self._lat_last
        if last is None:
            raise RuntimeError("latent_buffers: no evaluate_latent pass has run")
        if self.backend != "hip":
            return {k: v.clone() for k, v in last.items()}
        C, n = native.require(), last
        ws = self._lat_ws[1]
        return dict(mulv=self._lat_rows[:n].clone(), eps=C.latent_ws_view(ws[0], n, self.Z, None, "eps").clone(),
                    z=C.latent_ws_view(ws[0], n, self.Z, None, "z").clone())


class SampleEval:
    """Mixin: ``evaluate_samples``, the sample report (models/sample_report.py):
    kernel MMD and the 1-NN two-sample test between decoded prior samples and
    rows ``X[idx]``. The decoder runs through the trainer's ``decode`` (the
    Bernoulli mean the sample images show); the per-row table comes from the
    HIP kernels (csrc/kernels/two_sample.hip) on the hip backend and from the
    oracle's torch ops otherwise. Eager: three launches per pass.

    Requires ``self.Z``, ``self.seed``, ``self.device``, ``self.backend`` and
    ``self.decode(z) -> [n, D]``."""

    # elements per torch-backend block: [chunk, na + nb, D] float32 stays within 64 MiB
    SAMPLE_CHUNK_ELEMS = 1 << 24

    @torch.no_grad()
    def evaluate_samples(self, X: torch.Tensor, idx: torch.Tensor, n_samples=None, return_rows: bool = False) -> dict:
        """The sample report of ``n_samples`` decoded prior draws (default: as
        many as rows) against rows ``X[idx]``: ``dict(rows_real, rows_fake,
        mean_pair_d2, bandwidths, mmd2, mmd2_per_bandwidth, nn_acc, nn_acc_real,
        nn_acc_fake, nn_dist_real_to_fake, nn_dist_fake_to_real, rf_asym)``;
        with ``return_rows`` also ``table`` (float32 ``[rows_real + rows_fake,
        8]``), ``real`` and ``fake``. Training, eval, iw and latent state are not
        touched; the result depends on (weights, data, seed, n) only."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        na = idx.numel()
        nb = na if n_samples is None else int(n_samples)
        real = X[idx].to(self.device, torch.float32).reshape(na, -1).contiguous()
        D = real.shape[1]
        check_sample_args(na, nb, D)
        m = mean_pair_d2(real)
        h = bandwidths_of(m)
        z = torch.from_numpy(sample_z(nb, self.Z, self.seed)).to(self.device)
        fake = self.decode(z).to(torch.float32).reshape(nb, -1).contiguous()
        if self.backend != "hip":
            table = sample_rows(real, fake, h, chunk=max(1, self.SAMPLE_CHUNK_ELEMS // ((na + nb) * D)))
        else:
            C = native.require()
            # the workspace grows with (na + nb)^2 / 32 (58 MB at 20000 rows): it lives for this pass only
            ws = torch.empty(C.two_sample_ws_numel(na, nb, D), dtype=torch.float32, device=self.device)
            table = torch.empty(na + nb, COLS, dtype=torch.float32, device=self.device)
            C.two_sample_rows(real, fake, list(h), ws, table)
        out = dict(rows_real=na, rows_fake=nb, mean_pair_d2=m, bandwidths=list(h), **sample_stats(table, na, nb))
        if return_rows:
            out.update(table=table, real=real, fake=fake)
        return out
