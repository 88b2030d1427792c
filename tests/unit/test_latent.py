"""Latent report (models/latent.py, ``evaluate_latent``) on the torch backends,
the HPO runner and the CLI. The kernels' side is tests/gpu/test_latent_gpu.py;
inputs and bounds are tests/latent_cases.py.
"""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from multidisttorch_amd.data.datasets import synthetic_images
from multidisttorch_amd.models import iw, latent
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from multidisttorch_amd.ops.philox import reparam_eps
from tests import latent_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, N, SEED = 32, 85, 11
MIXED = [(85, 20), (117, 32), (53, 64)]


def _data(n=256):
    return synthetic_images(n, seed=3)


def _mlp(**kw):
    kw.setdefault("seed", SEED)
    kw.setdefault("batch_size", B)
    return MlpVaeTrainer(device="cpu", backend="torch", **kw)


def _conv(**kw):
    kw.setdefault("seed", SEED)
    kw.setdefault("batch_size", B)
    return ConvVaeTrainer(image=28, z=32, device="cpu", backend="torch", **kw)


def _train(tr, X, steps):
    tr.bind_train_data(X, torch.arange(X.shape[0], dtype=torch.int32))
    tr.set_cursor(0, X.shape[0] // tr.B)
    tr.train_steps(steps)


def _eps(n, Z, seed=SEED):
    return torch.from_numpy(latent.latent_eps(n, Z, seed))


def _cases():
    return [("overlap", lc.overlap())] + [(f"mixed{n}x{Z}", lc.mixed(n, Z)) for n, Z in MIXED] + \
           [(f"sharp{n}x{Z}", lc.sharp(n, Z)) for n, Z in MIXED]


def test_stream_word_and_eps_definition():
    assert latent.LATENT_STREAM == 3 << 28 and latent.LATENT_STREAM not in (iw.IW_STREAM, 1 << 30)
    np.testing.assert_array_equal(latent.latent_eps(7, 5, SEED), reparam_eps(7, 5, SEED, 3 << 28, 0))


@pytest.mark.parametrize("name,mulv", _cases(), ids=[c[0] for c in _cases()])
def test_split_sums_to_the_sampled_kl(name, mulv):
    n, Z = mulv.shape[0], mulv.shape[1] // 2
    o = lc.oracle(mulv, _eps(n, Z))
    assert abs(o["mi"] + o["tc"] + o["dwkl"] - o["sampled_kl"]) <= 1e-12 * max(1.0, abs(o["sampled_kl"]))
    assert o["mi"] <= math.log(n) + 1e-12
    assert abs(o["kl"] - float(o["kl_per_dim"].sum())) <= 1e-12 * o["kl"]
    # chunking over i changes nothing but the blocking
    c = lc.oracle(mulv, _eps(n, Z), chunk=7)
    for k in lc.SCALARS:
        assert abs(c[k] - o[k]) <= 1e-11 * max(1.0, abs(o[k])), k
    np.testing.assert_allclose(c["lq_marg"].numpy(), o["lq_marg"].numpy(), rtol=1e-12)


def test_overlap_case_keeps_mi_off_the_ceiling():
    mulv = lc.overlap()
    o = lc.oracle(mulv, _eps(40, 4))
    assert 0.0 < o["mi"] < 0.8 * math.log(40)
    assert o["active_units"] == 1


@pytest.mark.parametrize("n,Z", MIXED)
def test_active_units_exact_on_mixed(n, Z):
    mulv = lc.mixed(n, Z)
    for dtype in (torch.float64, torch.float32):
        o = lc.oracle(mulv, _eps(n, Z), dtype)
        assert o["active_units"] == Z // 4
        mv = o["mu_var"].double()
        assert float(mv[: Z // 4].min()) > 1.0 and float(mv[Z // 4:].max()) < 0.005
    # the threshold is the caller's
    assert lc.oracle(mulv, _eps(n, Z), au_threshold=1e-4)["active_units"] == Z
    assert lc.oracle(mulv, _eps(n, Z), au_threshold=50.0)["active_units"] == 0


def test_sharp_case_needs_the_max_subtraction():
    mulv = lc.sharp(53, 64)
    assert lc.max_joint(mulv, _eps(53, 64)) > 88.7
    o = lc.oracle(mulv, _eps(53, 64), torch.float32)
    assert all(math.isfinite(o[k]) for k in lc.SCALARS)


def test_one_row_has_no_mi_and_no_tc():
    mulv = lc.mixed(1, 20)
    for dtype in (torch.float64, torch.float32):
        o = lc.oracle(mulv, _eps(1, 20), dtype)
        assert o["mi"] == 0.0 and o["tc"] == 0.0 and o["dwkl"] == o["sampled_kl"]
        assert o["active_units"] == 0 and float(o["mu_var"].abs().max()) == 0.0


def test_identical_rows_carry_no_information():
    mulv = lc.mixed(1, 20).expand(30, 40).contiguous()
    o = lc.oracle(mulv, _eps(30, 20))
    assert abs(o["mi"]) < 1e-12 and o["active_units"] == 0


def _trainer_oracle(tr):
    buf = tr.latent_buffers()
    return buf, lc.bounds(buf["mulv"], buf["eps"])


@pytest.mark.parametrize("make,steps", [(_mlp, 0), (_mlp, 30), (_conv, 3)], ids=["mlp0", "mlp30", "conv3"])
def test_torch_backend_matches_float64_oracle(make, steps):
    X = _data()
    tr = make()
    if steps:
        _train(tr, X, steps)
    r = tr.evaluate_latent(X, torch.arange(N), return_rows=True)
    assert set(r) == {"rows", "kl", "kl_per_dim", "mu_var", "post_var", "active_units", "au_threshold", "mi", "tc",
                      "dwkl", "sampled_kl", "lq_joint", "lq_marg", "lq_cond", "lp"}
    assert "lq_joint" not in tr.evaluate_latent(X, torch.arange(N))
    buf, (o64, bound) = _trainer_oracle(tr)
    assert buf["mulv"].shape == (N, 2 * tr.Z) and buf["mulv"].dtype == torch.float32
    np.testing.assert_array_equal(buf["eps"].numpy(), reparam_eps(N, tr.Z, SEED, 3 << 28, 0))
    mu, lv = buf["mulv"][:, :tr.Z], buf["mulv"][:, tr.Z:]
    np.testing.assert_allclose(buf["z"].numpy(), (mu + buf["eps"] * torch.exp(0.5 * lv)).numpy(), rtol=1e-6, atol=1e-7)
    lc.check(r, o64, bound, f"{type(tr).__name__} torch")
    # the encoder rows are the model's
    if isinstance(tr, MlpVaeTrainer):
        m2, l2 = iw.mlp_encode(tr.named_parameters(), X[:N])
    else:
        m2, l2 = tr.model.encode(X[:N])
    np.testing.assert_allclose(buf["mulv"].numpy(), torch.cat([m2, l2], 1).detach().numpy(), rtol=1e-5, atol=1e-6)


def test_chunked_pass_matches_unchunked():
    X = _data()
    tr = _mlp()
    a = tr.evaluate_latent(X, torch.arange(N), return_rows=True)
    tr.LATENT_CHUNK_ELEMS = 5 * N * tr.Z  # 5 rows i per block
    b = tr.evaluate_latent(X, torch.arange(N), return_rows=True)
    for k in lc.SCALARS:
        assert abs(a[k] - b[k]) <= 2e-5 * max(1.0, abs(a[k])), k
    np.testing.assert_allclose(a["lq_marg"].numpy(), b["lq_marg"].numpy(), rtol=1e-5)


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_result_depends_on_weights_data_seed_and_n_only(make):
    X = _data()
    idx = torch.arange(N)
    base = make().evaluate_latent(X, idx, return_rows=True)
    for kw in (dict(batch_size=16), dict(kl_beta=4.0), dict(rng_stream=3)):
        r = make(**kw).evaluate_latent(X, idx, return_rows=True)
        for k in lc.SCALARS:
            assert abs(r[k] - base[k]) <= 1e-5 * max(1.0, abs(base[k])), (kw, k)
        np.testing.assert_allclose(r["lq_joint"].numpy(), base["lq_joint"].numpy(), rtol=2e-5, atol=2e-5)
        assert r["active_units"] == base["active_units"]
    r = make(rng_stream=3).evaluate_latent(X, idx, return_rows=True)
    assert all(r[k] == base[k] for k in lc.SCALARS) and torch.equal(r["lq_marg"], base["lq_marg"])
    other = make(seed=SEED + 1, init_seed=SEED).evaluate_latent(X, idx)
    assert other["kl"] == base["kl"] and other["mi"] != base["mi"]  # the seed draws eps; kl is analytic


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_pass_leaves_train_eval_and_iw_state_alone(make):
    X = _data()
    tr = make()
    _train(tr, X, 2)
    tr.evaluate(X, torch.arange(N), want_first_recon=False)
    iw0 = tr.evaluate_iw(X, torch.arange(N), 2)
    before = (tr.read_state(), tr.read_state(eval=True), tr.loss_history().copy(), tr.loss_history(eval=True).copy())
    tr.evaluate_latent(X, torch.arange(N))
    after = (tr.read_state(), tr.read_state(eval=True), tr.loss_history(), tr.loss_history(eval=True))
    assert before[0] == after[0] and before[1] == after[1]
    np.testing.assert_array_equal(before[2], after[2])
    np.testing.assert_array_equal(before[3], after[3])
    assert tr.evaluate_iw(X, torch.arange(N), 2) == iw0


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_training_continues_bitwise_after_a_pass(make):
    X = _data()
    a, b = make(), make()
    _train(a, X, 6)
    _train(b, X, 3)
    b.evaluate_latent(X, torch.arange(N))
    b.train_steps(3)
    for n in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert a.read_state() == b.read_state()


def test_argument_validation():
    X = _data()
    tr = _mlp()
    with pytest.raises(ValueError):
        tr.evaluate_latent(X, torch.arange(0))
    with pytest.raises(ValueError):
        tr.evaluate_latent(X, torch.arange(N), au_threshold=-1.0)
    with pytest.raises(ValueError):
        latent.check_latent_args(10, 65)
    with pytest.raises(ValueError):
        latent.check_latent_args(10, 0)
    with pytest.raises(ValueError):
        latent.check_latent_args(2 ** 32 // 64 + 1, 64)
    latent.check_latent_args(2 ** 32 // 64, 64)
    with pytest.raises(RuntimeError):
        _mlp().latent_buffers()


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


def test_cli_reports_latent_only_when_asked(tmp_path):
    out, agg, recs, agg_file = _cli(tmp_path, 29681, "--latent-report", "--au-threshold", "0.02")
    m = re.search(r"====> Test set latent: KL ([0-9.]+) active (\d+)/(\d+) MI ([0-9.]+) TC (-?[0-9.]+) DWKL (-?[0-9.]+)$",
                  out, re.M)
    assert m, out[-2000:]
    kl, au, Z, mi = float(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4))
    assert Z == 20 and 0 <= au <= Z and kl > 0 and 0 <= mi <= math.log(85) + 1e-3
    assert set(agg["latent"]) == {"0"} and set(agg["latent"]["0"]) == {"kl", "active_units", "mi", "tc", "dwkl"}
    assert agg["latent"]["0"]["active_units"] == au and abs(agg["latent"]["0"]["kl"] - kl) < 1e-4
    assert agg_file == agg
    rec = [r for r in recs if r.get("event") == "latent_eval"]
    assert len(rec) == 1 and rec[0]["latent_s"] > 0 and rec[0]["rows"] == 85 and rec[0]["au_threshold"] == 0.02
    assert {"kl", "kl_per_dim", "mu_var", "post_var", "active_units", "mi", "tc", "dwkl", "sampled_kl"} <= set(rec[0])
    assert len(rec[0]["kl_per_dim"]) == 20 and abs(sum(rec[0]["kl_per_dim"]) - rec[0]["kl"]) < 1e-3
    assert abs(rec[0]["mi"] + rec[0]["tc"] + rec[0]["dwkl"] - rec[0]["sampled_kl"]) < 1e-4
    out0, agg0, recs0, _ = _cli(tmp_path, 29682)
    assert "latent" not in out0
    assert not [k for k in agg0 if "latent" in k]
    assert not [r for r in recs0 if any("latent" in k for k in r) or r.get("event") == "latent_eval"]
    # everything before the pass is what the run prints without the flag
    drop = ("Done. time", "MDT_AGGREGATE", "Test set latent", "master at", "[Gloo]")  # timings, the port, the new line
    strip = lambda s: [l for l in s.splitlines() if not any(d in l for d in drop)]
    assert strip(out) == strip(out0)
