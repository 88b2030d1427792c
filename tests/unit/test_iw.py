"""Importance-weighted test log-likelihood (models/iw.py, ``evaluate_iw``) on
the torch backends, the HPO runner and the CLI. The kernels' side is
tests/gpu/test_iw_gpu.py.

Bounds: the fp32 pass against the float64 oracle is held to rel 2e-5 per row,
the project's bound for an fp32 loss against an oracle of the same math; fp32
rounding of the ~540-nat row sums measured 1.5e-7. The conv trainer's torch
backend computes in fp32 as well (stock torch ops), so the same bound holds
there; its oracle is the same module in float64.
"""
import copy
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from multidisttorch_amd.data.datasets import synthetic_images
from multidisttorch_amd.models import iw
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from multidisttorch_amd.models.mlp_vae import _bce_terms
from multidisttorch_amd.ops.philox import reparam_eps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, N, SEED = 32, 85, 11
REL = 2e-5


def _data(n=256):
    return synthetic_images(n, seed=3)


def _mlp(**kw):
    kw.setdefault("seed", SEED)
    return MlpVaeTrainer(batch_size=B, device="cpu", backend="torch", **kw)


def _conv(**kw):
    kw.setdefault("seed", SEED)
    return ConvVaeTrainer(batch_size=B, image=28, z=32, device="cpu", backend="torch", **kw)


def _train(tr, X, steps):
    tr.bind_train_data(X, torch.arange(X.shape[0], dtype=torch.int32))
    tr.set_cursor(0, X.shape[0] // B)
    tr.train_steps(steps)


def _host_eps(K, Z, b, M):
    """The issue's definition, spelled out: reparam_eps(K*B, Z, seed, 1 << 29, b).reshape(K, B, Z)."""
    return torch.from_numpy(reparam_eps(K * B, Z, SEED, 1 << 29, b).reshape(K, B, Z)[:, :M].copy()).double()


def _oracle_rows(logw_fn, X, n, K, Z):
    rn, re_ = [], []
    for b in range(-(-n // B)):
        M = min(B, n - b * B)
        a, e = iw.iw_reduce(logw_fn(X[b * B: b * B + M].double(), _host_eps(K, Z, b, M)))
        rn.append(a)
        re_.append(e)
    return torch.cat(rn), torch.cat(re_)


def _mlp_oracle(tr, X, n, K):
    v = {k: t.detach().double() for k, t in tr.named_parameters().items()}
    return _oracle_rows(lambda x, eps: iw.mlp_iw_log_weights(v, x, eps)[0], X, n, K, tr.Z)


def _conv_oracle(tr, X, n, K):
    m = copy.deepcopy(tr.model).double()

    def logw(x, eps):
        with torch.no_grad():
            mu, lv = m.encode(x)
            dec = lambda z: m.decode_logits(z).permute(0, 2, 3, 1).reshape(z.shape[0], -1)
            return iw.iw_log_weights(mu, lv, eps, x, dec)[0]

    return _oracle_rows(logw, X, n, K, tr.Z)


def _check_rows(r, rn, re_, n, K):
    assert r["rows"] == n and r["k"] == K
    assert r["row_nll"].dtype == torch.float32 and r["row_nll"].shape == (n,)
    np.testing.assert_allclose(r["row_nll"].double().numpy(), rn.numpy(), rtol=REL, atol=0)
    np.testing.assert_allclose(r["row_neg_elbo"].double().numpy(), re_.numpy(), rtol=REL, atol=0)
    assert abs(r["nll"] - float(rn.sum())) <= REL * float(rn.sum())
    assert abs(r["neg_elbo"] - float(re_.sum())) <= REL * float(re_.sum())


@pytest.mark.parametrize("K,chunk", [(5, 2), (1, None)])
@pytest.mark.parametrize("steps", [0, 30])
def test_mlp_torch_backend_matches_float64_oracle(K, chunk, steps):
    X = _data()
    tr = _mlp()
    if steps:
        _train(tr, X, steps)
    r = tr.evaluate_iw(X, torch.arange(N), K, chunk_samples=chunk, return_rows=True)
    _check_rows(r, *_mlp_oracle(tr, X, N, K), N, K)
    # a spread of several nats over k: the reduction has to subtract the max
    assert float(r["row_nll"].min()) > 100.0


@pytest.mark.parametrize("K,chunk", [(5, 2), (1, None)])
def test_conv_torch_backend_matches_float64_oracle(K, chunk):
    X = _data()
    tr = _conv()
    _train(tr, X, 3)
    r = tr.evaluate_iw(X, torch.arange(N), K, chunk_samples=chunk, return_rows=True)
    _check_rows(r, *_conv_oracle(tr, X, N, K), N, K)


def test_chunking_does_not_change_the_result():
    X = _data()
    tr = _mlp()
    idx = torch.arange(N)
    a = tr.evaluate_iw(X, idx, 5, chunk_samples=2, return_rows=True)
    b = tr.evaluate_iw(X, idx, 5, return_rows=True)
    np.testing.assert_allclose(a["row_nll"].numpy(), b["row_nll"].numpy(), rtol=1e-6)
    assert "row_nll" not in tr.evaluate_iw(X, idx, 5)


@pytest.mark.parametrize("K", [1, 4])
def test_mlp_degenerate_identity(K):
    """fc21 = fc22 = 0 and fc3.weight = 0: mu = lv = 0, z = eps, the decoder
    ignores z, so every logw is -bce(x; constant logits) and both bounds equal
    that BCE for every K."""
    X = _data()
    tr = _mlp()
    v = tr.named_parameters()
    for n in ("fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias", "fc3.weight"):
        v[n].zero_()
    r = tr.evaluate_iw(X, torch.arange(N), K, chunk_samples=3, return_rows=True)
    vd = {k: t.double() for k, t in v.items()}
    t = torch.relu(vd["fc3.bias"]) @ vd["fc4.weight"].t() + vd["fc4.bias"]
    bce = _bce_terms(t.unsqueeze(0), X[:N].double()).sum(-1)
    np.testing.assert_allclose(r["row_nll"].double().numpy(), bce.numpy(), rtol=REL, atol=0)
    np.testing.assert_allclose(r["row_neg_elbo"].double().numpy(), bce.numpy(), rtol=REL, atol=0)


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_jensen(make):
    X = _data()
    tr = make()
    _train(tr, X, 3)
    idx = torch.arange(N)
    r = tr.evaluate_iw(X, idx, 6, return_rows=True)
    assert bool((r["row_nll"] <= r["row_neg_elbo"] + 1e-3).all())
    assert r["nll"] < r["neg_elbo"]
    r1 = tr.evaluate_iw(X, idx, 1, return_rows=True)
    np.testing.assert_allclose(r1["row_nll"].numpy(), r1["row_neg_elbo"].numpy(), rtol=0, atol=1e-3)


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_replicas_agree(make):
    X = _data()
    out = []
    for stream in (0, 3):
        tr = make(rng_stream=stream)
        r = tr.evaluate_iw(X, torch.arange(N), 3, return_rows=True)
        out.append(r)
    assert out[0]["nll"] == out[1]["nll"] and out[0]["neg_elbo"] == out[1]["neg_elbo"]
    assert torch.equal(out[0]["row_nll"], out[1]["row_nll"])


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_pass_leaves_train_and_eval_state_alone(make):
    X = _data()
    tr = make()
    _train(tr, X, 2)
    tr.evaluate(X, torch.arange(N), want_first_recon=False)
    before = (tr.read_state(), tr.read_state(eval=True), tr.loss_history().copy(), tr.loss_history(eval=True).copy())
    tr.evaluate_iw(X, torch.arange(N), 3)
    after = (tr.read_state(), tr.read_state(eval=True), tr.loss_history(), tr.loss_history(eval=True))
    assert before[0] == after[0] and before[1] == after[1]
    np.testing.assert_array_equal(before[2], after[2])
    np.testing.assert_array_equal(before[3], after[3])


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_training_continues_bitwise_after_a_pass(make):
    X = _data()
    a, b = make(), make()
    _train(a, X, 6)
    _train(b, X, 3)
    b.evaluate_iw(X, torch.arange(N), 3, chunk_samples=2)
    b.train_steps(3)
    for n in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert a.read_state() == b.read_state()


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_argument_validation(make):
    X = _data()
    tr = make()
    idx = torch.arange(N)
    with pytest.raises(ValueError):
        tr.evaluate_iw(X, idx, 0)
    with pytest.raises(ValueError):
        tr.evaluate_iw(X, idx, 2 ** 32 // (B * tr.Z) + 1)
    with pytest.raises(ValueError):
        tr.evaluate_iw(X, idx, 3, chunk_samples=0)


def _cli(tmp_path, port, *extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
    mdir = os.path.join(str(tmp_path), "m" + str(port))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vae-hpo.py"), "--ngroups", "1", "--backend", "torch",
                        "--epochs", "1", "--train-samples", "256", "--test-samples", "85", "--batch-size", "32",
                        "--no-results", "--metrics-dir", mdir, *extra],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    with open(os.path.join(mdir, "trial-0.jsonl")) as f:
        recs = [json.loads(l) for l in f]
    with open(os.path.join(mdir, "aggregate.json")) as f:
        agg_file = json.load(f)
    return r.stdout, json.loads(re.search(r"MDT_AGGREGATE (.*)", r.stdout).group(1)), recs, agg_file


def test_cli_reports_iw_only_when_asked(tmp_path):
    out, agg, recs, agg_file = _cli(tmp_path, 29671, "--iw-samples", "4")
    m = re.search(r"====> Test set IW-4 NLL: ([0-9.]+) ELBO-4: ([0-9.]+)", out)
    assert m, out[-2000:]
    nll, ne = float(m.group(1)), float(m.group(2))
    assert 0 < nll < ne
    assert agg["iw_samples"] == 4 and agg["best_trial_by_iw_nll"] == 0
    assert agg["iw_nll"] == {"0": nll}
    assert agg_file == agg
    rec = [r for r in recs if r.get("event") == "iw_eval"]
    assert len(rec) == 1 and rec[0]["iw_samples"] == 4 and rec[0]["iw_s"] > 0
    assert abs(rec[0]["iw_nll"] - nll) < 1e-4 and abs(rec[0]["iw_neg_elbo"] - ne) < 1e-4
    out0, agg0, recs0, _ = _cli(tmp_path, 29672)
    assert "IW-" not in out0
    assert not [k for k in agg0 if "iw" in k]
    assert not [r for r in recs0 if any("iw" in k for k in r) or r.get("event") == "iw_eval"]
    # everything before the pass is what the run prints without the flag
    drop = ("Done. time", "MDT_AGGREGATE", "IW-", "master at", "[Gloo]")  # timings, the port, the new lines
    strip = lambda s: [l for l in s.splitlines() if not any(d in l for d in drop)]
    assert strip(out) == strip(out0)

