"""Importance-weighted test log-likelihood on the HIP backends
(csrc/kernels/vae_iw.hip, conv_iw.hip; ``evaluate_iw`` of both trainers).

Bounds, none of them taken from the code under test:
  * MLP rows against the float64 oracle (models/iw.py on host eps): rel 2e-5,
    the project's bound for HIP-vs-torch eval losses
    (test_eval_loss_with_tail_batch_matches_torch_backend);
  * device eps against host ``reparam_eps``: rtol = atol = 1e-5, as
    test_philox_host_matches_device;
  * conv rows against a float64 recomputation that shares the pass's bf16
    rounding points (same decoder kernels on the same latents): rel 1e-4
    (test_conv28_fused.py), and per row the derived reduce bound of
    tests/iw_checker.py on the recomputed log-weights, with the BCE and prior
    bounds carried (about 1e-4 nat absolute at |logw| ~ 540);
  * conv degenerate identity against ``evaluate()``: rel 1e-3, the layer
    path's loss bound (test_conv_vae_kernels.py).
The log-weights sit near -540 (MLP, fresh weights) with a spread of several
nats over k, so a reduction without max-subtraction underflows here.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 7


def _dev():
    return torch.device("cuda", 0)


_cache = {}


def _images(n, size=28):
    from multidisttorch_amd.data.datasets import synthetic_images

    key = (n, size)
    if key not in _cache:
        _cache[key] = synthetic_images(n, size=size, seed=5, device=_dev())
    return _cache[key]


def _mlp(B=32, graphs=False, **kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    return MlpVaeTrainer(batch_size=B, device=_dev(), backend="hip", seed=SEED, use_graphs=graphs, graph_steps=3, **kw)


def _conv(B=32, image=28, graphs=False, **kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    return ConvVaeTrainer(batch_size=B, image=image, z=32 if image == 28 else 64, device=_dev(), backend="hip",
                          seed=SEED, use_graphs=graphs, graph_steps=3, **kw)


def _train(tr, X, steps):
    n = X.shape[0] // tr.B * tr.B
    tr.bind_train_data(X, torch.arange(n, dtype=torch.int32, device=X.device))
    tr.set_cursor(0, n // tr.B)
    tr.train_steps(steps)
    torch.cuda.synchronize()


def _host_eps(K, B, Z, b):
    from multidisttorch_amd.ops.philox import reparam_eps

    return reparam_eps(K * B, Z, SEED, 1 << 29, b).reshape(K, B, Z)


def _arange(n):
    return torch.arange(n, dtype=torch.int32, device=_dev())


@pytest.mark.parametrize("n,K,chunk", [(85, 5, 2), (33, 5, 2), (85, 1, None)])
def test_mlp_rows_match_float64_oracle(n, K, chunk, native_ext):
    from multidisttorch_amd.models.iw import iw_reduce, mlp_iw_log_weights

    B = 32
    X = _images(256)
    tr = _mlp(B)
    _train(tr, X, 30)
    r = tr.evaluate_iw(X, _arange(n), K, chunk_samples=chunk, return_rows=True)
    torch.cuda.synchronize()
    # the last batch's last chunk, as drawn on the device
    nb = -(-n // B)
    M = n - (nb - 1) * B
    S = chunk or K
    k0 = (K - 1) // S * S
    buf = tr.iw_buffers(K - k0, M)
    np.testing.assert_allclose(buf["eps"].cpu().numpy(), _host_eps(K, B, tr.Z, nb - 1)[k0:, :M], rtol=1e-5, atol=1e-5)
    v = {k: t.detach().cpu().double() for k, t in tr.named_parameters().items()}
    rn, re_ = [], []
    for b in range(nb):
        m = min(B, n - b * B)
        eps = torch.from_numpy(_host_eps(K, B, tr.Z, b)[:, :m].copy()).double()
        logw, z = mlp_iw_log_weights(v, X[b * B: b * B + m].cpu().double(), eps)
        a, e = iw_reduce(logw)
        rn.append(a)
        re_.append(e)
    rn, re_ = torch.cat(rn), torch.cat(re_)
    np.testing.assert_allclose(buf["z"].cpu().numpy(), z[k0:].numpy(), rtol=1e-4, atol=1e-5)
    print("max rel err row_nll", float(((r["row_nll"].cpu().double() - rn).abs() / rn).max()),
          "row_neg_elbo", float(((r["row_neg_elbo"].cpu().double() - re_).abs() / re_).max()))
    assert r["rows"] == n and r["k"] == K and r["row_nll"].dtype == torch.float32
    np.testing.assert_allclose(r["row_nll"].cpu().double().numpy(), rn.numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(r["row_neg_elbo"].cpu().double().numpy(), re_.numpy(), rtol=2e-5, atol=0)
    assert abs(r["nll"] - float(rn.sum())) <= 2e-5 * float(rn.sum())
    assert abs(r["neg_elbo"] - float(re_.sum())) <= 2e-5 * float(re_.sum())
    if K > 1:
        assert bool((r["row_nll"] <= r["row_neg_elbo"] + 1e-3).all())


@pytest.mark.parametrize("K", [1, 5])
def test_mlp_degenerate_identity(K, native_ext):
    """mu = lv = 0 and a decoder that ignores z: both bounds are the BCE of the
    constant logits, for every K."""
    from multidisttorch_amd.models.mlp_vae import _bce_terms

    n = 85
    X = _images(256)
    tr = _mlp(32)
    v = tr.named_parameters()
    for name in ("fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias", "fc3.weight"):
        v[name].zero_()
    r = tr.evaluate_iw(X, _arange(n), K, chunk_samples=2, return_rows=True)
    torch.cuda.synchronize()
    vd = {k: t.cpu().double() for k, t in v.items()}
    t = torch.relu(vd["fc3.bias"]) @ vd["fc4.weight"].t() + vd["fc4.bias"]
    bce = _bce_terms(t.unsqueeze(0), X[:n].cpu().double()).sum(-1)
    np.testing.assert_allclose(r["row_nll"].cpu().double().numpy(), bce.numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(r["row_neg_elbo"].cpu().double().numpy(), bce.numpy(), rtol=2e-5, atol=0)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_graphed_pass_is_bitwise_eager_and_repeatable(kind, native_ext):
    X = _images(256)
    n, K = 117, 3  # batches 32, 32, 32 (one graph of two) and a tail of 21 (a graph of its own)
    out = {}
    for graphs in (False, True):
        tr = _mlp(32, graphs) if kind == "mlp" else _conv(32, 28, graphs)
        _train(tr, X, 3)
        res = []
        for _ in range(2):
            r = tr.evaluate_iw(X, _arange(n), K, chunk_samples=2, return_rows=True)
            torch.cuda.synchronize()
            res.append((r["nll"], r["neg_elbo"], r["row_nll"].cpu(), r["row_neg_elbo"].cpu()))
        out[graphs] = res
        if graphs:
            assert len(tr._iw_graphs) == 2, "the graphed path did not run"
    a0, a1 = out[False]
    for b in (a1, *out[True]):
        assert a0[0] == b[0] and a0[1] == b[1], (a0[:2], b[:2])
        assert torch.equal(a0[2], b[2]) and torch.equal(a0[3], b[3])
    assert np.isfinite(a0[0]) and a0[0] < a0[1]


def test_mlp_graphs_survive_a_larger_chunk(native_ext):
    """A pass with more samples per chunk makes the engine's chunk workspace
    grow; graphs captured over the old one must not be replayed."""
    X = _images(256)
    tr = _mlp(32, True)
    idx = _arange(117)
    a = tr.evaluate_iw(X, idx, 3, chunk_samples=1, return_rows=True)
    cap = tr.engine.iw_capacity()
    b = tr.evaluate_iw(X, idx, 6, return_rows=True)  # one chunk of 6 samples: a larger workspace
    assert tr.engine.iw_capacity() > cap
    c = tr.evaluate_iw(X, idx, 3, chunk_samples=1, return_rows=True)
    torch.cuda.synchronize()
    assert a["nll"] == c["nll"] and torch.equal(a["row_nll"], c["row_nll"])
    assert torch.equal(a["row_neg_elbo"], c["row_neg_elbo"])
    assert b["k"] == 6 and b["rows"] == 117


def _conv_recompute(tr, X, idx, K, chunk):
    """float64 log-weights ``lw[K, M]`` of the LAST batch of the pass over
    X[idx] and their bound, from what the pass exposes: mulv, and eps / z of
    the last chunk. The noise of sample k does not depend on K, so passes with
    K' = the chunk ends expose every chunk in turn. Each chunk's z goes through
    ``tr.decode()`` packed as the pass packs it (the same decoder kernels on the
    same bf16 latents in the same launch shapes: the same logits); BCE and prior
    term are redone in float64 with the bounds of tests/iw_checker.py. Also
    ``rolled``: lw with the image rows rolled by one (None when M = 1)."""
    from multidisttorch_amd.models.iw import default_chunk
    from tests import iw_checker as ck

    B, n = tr.B, idx.numel()
    nb = -(-n // B)
    M = n - (nb - 1) * B
    Sc = max(1, min(default_chunk(K, B, chunk), B // M))
    x = X[idx[(nb - 1) * B:].long()].cpu()
    host = _host_eps(K, B, tr.Z, nb - 1)
    lw, b_lw, rolled = [], [], []
    for k0 in range(0, K, Sc):
        k1 = min(k0 + Sc, K)
        s = k1 - k0
        tr.evaluate_iw(X, idx, k1, chunk_samples=chunk)
        torch.cuda.synchronize()
        buf = tr.iw_buffers(s, M)
        np.testing.assert_allclose(buf["eps"].cpu().numpy(), host[k0:k1, :M], rtol=1e-5, atol=1e-5)
        z, bz, prior, bp = ck.reparam_ref(buf["mulv"].cpu(), buf["eps"].cpu())
        assert ck.ratio(buf["z"].cpu(), z, bz) <= 1
        tr.decode(buf["z"].reshape(s * M, tr.Z))
        t = tr.logits[: s * M * tr.D].view(s * M, tr.D).cpu()
        bce, bb = ck.row_bce_ref(t, x, ck.conv_depth(tr.D))
        a, b = ck.lw_ref(prior, bce.view(s, M), bp, bb.view(s, M))
        lw.append(a)
        b_lw.append(b)
        if M > 1:
            rolled.append(prior - ck.row_bce_ref(t, x.roll(1, 0), ck.conv_depth(tr.D))[0].view(s, M))
    return torch.cat(lw), torch.cat(b_lw), torch.cat(rolled) if rolled else None


def _check_composition(tr, X, n, K, chunk, five_percent):
    from multidisttorch_amd.models.iw import iw_reduce
    from tests import iw_checker as ck

    B = tr.B
    idx = _arange(n)
    r = tr.evaluate_iw(X, idx, K, chunk_samples=chunk, return_rows=True)
    torch.cuda.synchronize()
    rows = (r["row_nll"].cpu().double(), r["row_neg_elbo"].cpu().double())
    # batch 0 alone is the same function of (weights, data, seed, K)
    r0 = tr.evaluate_iw(X, idx[:B], K, chunk_samples=chunk, return_rows=True)
    assert torch.equal(r0["row_nll"].cpu(), r["row_nll"][:B].cpu())
    for lo, sub in ((0, idx[:B]), (n - n % B, idx)):
        lw, b_lw, rolled = _conv_recompute(tr, X, sub, K, chunk)
        rn, re_ = iw_reduce(lw)
        m = rn.numel()
        print("rows", lo, "max rel err", float(((rows[0][lo:lo + m] - rn).abs() / rn).max()),
              float(((rows[1][lo:lo + m] - re_).abs() / re_).max()), "row spread", float(rn.max() - rn.min()))
        np.testing.assert_allclose(rows[0][lo:lo + m].numpy(), rn.numpy(), rtol=1e-4, atol=0)
        np.testing.assert_allclose(rows[1][lo:lo + m].numpy(), re_.numpy(), rtol=1e-4, atol=0)
        # the reduce bound of tests/iw_checker.py on the recomputed log-weights, b_lw from the BCE and prior bounds
        nll, ne, bn, be = ck.reduce_ref(lw, b_lw)
        ra, rb = ck.ratio(rows[0][lo:lo + m], nll, bn), ck.ratio(rows[1][lo:lo + m], ne, be)
        print(f"RATIO conv_pass.row_nll {ra:.4g} conv_pass.row_neg_elbo {rb:.4g} (n={n} K={K} rows {lo}..)")
        assert ra <= 1 and rb <= 1, (ra, rb)
        # a mispaired image row would show at every row: the oracle with the rows rolled by one leaves the bound
        n2, e2, _, _ = ck.reduce_ref(rolled)   # (every batch here has more than one row)
        assert bool((((n2 - nll).abs() > bn) | ((e2 - ne).abs() > be)).all()), "rows too alike to tell a mispaired sample"
        if five_percent:
            assert float(rn.max() - rn.min()) > 0.05 * float(rn.mean()), "rows too alike to tell a mispaired sample"
    for name, tot in (("nll", rows[0]), ("neg_elbo", rows[1])):
        rt = ck.totals_ratio(r[name], tot.float())
        print(f"RATIO conv_pass.total_{name} {rt:.4g}")
        assert rt <= 1
    assert bool((r["row_nll"] <= r["row_neg_elbo"] + 1e-3).all())


# tail 21: chunks of 1; tail 5: chunks of 2; tail 5 with the default chunk: 6 samples per chunk, the last chunk holds 2
@pytest.mark.parametrize("n,K,chunk", [(53, 3, 2), (37, 4, 2), (37, 50, None)])
def test_conv28_composition(n, K, chunk, native_ext):
    X = _images(256)
    tr = _conv(32, 28)
    assert tr.f28, "MDT_CONV_F28 default: training runs the fused step, the pass the layer path"
    _train(tr, X, 40)
    _check_composition(tr, X, n, K, chunk, five_percent=True)


def test_conv128_composition(native_ext):
    """The same at 128 x 128, B = 16, Z = 64: a tail of 5 in chunks of 2 (n = 21, K = 3, chunk = 2)."""
    X = _images(64, 128)
    tr = _conv(16, 128)
    _train(tr, X, 10)
    _check_composition(tr, X, 21, 3, 2, five_percent=False)


@pytest.mark.parametrize("image,B,n", [(28, 32, 53), (128, 16, 21)])
def test_conv_degenerate_identity(image, B, n, native_ext):
    """enc_head = 0 and dec_fc.weight = 0: mu = lv = 0 (KLD 0) and constant
    logits, so the pass's nll is ``evaluate()``'s total."""
    X = _images(64, image)
    tr = _conv(B, image)
    v = tr.named_parameters()
    for name in ("enc_head.weight", "enc_head.bias", "dec_fc.weight"):
        v[name].zero_()
    tr.refresh_weights()
    total, _ = tr.evaluate(X, _arange(n), want_first_recon=False)
    r = tr.evaluate_iw(X, _arange(n), 3, chunk_samples=2)
    torch.cuda.synchronize()
    print("evaluate", total, "iw nll", r["nll"], "neg_elbo", r["neg_elbo"])
    assert abs(r["nll"] - total) <= 1e-3 * total
    assert abs(r["neg_elbo"] - total) <= 1e-3 * total


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_training_continues_bitwise_after_a_pass(kind, native_ext):
    """3 steps, one pass, 3 steps == 6 steps, bitwise (graph-replayed steps;
    conv: the fused 28x28 step with its next-batch prefetch and deferred
    transposed-weight copies), and the pass leaves both states and loss rings alone."""
    X = _images(256)
    make = (lambda: _mlp(32, True)) if kind == "mlp" else (lambda: _conv(32, 28, True))
    a, b = make(), make()
    _train(a, X, 6)
    _train(b, X, 3)
    b.evaluate(X, _arange(53), want_first_recon=False)
    torch.cuda.synchronize()
    before = (b.read_state(), b.read_state(eval=True), b.loss_history().copy(), b.loss_history(eval=True).copy())
    b.evaluate_iw(X, _arange(53), 3, chunk_samples=2)
    torch.cuda.synchronize()
    after = (b.read_state(), b.read_state(eval=True), b.loss_history(), b.loss_history(eval=True))
    assert before[0] == after[0] and before[1] == after[1]
    np.testing.assert_array_equal(before[2], after[2])
    np.testing.assert_array_equal(before[3], after[3])
    b.train_steps(3)
    torch.cuda.synchronize()
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.read_state() == b.read_state()
