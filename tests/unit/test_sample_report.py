"""Sample report (models/sample_report.py, ``evaluate_samples``) on the torch
backends and in the runner. The kernels' side is tests/gpu/test_two_sample_kernels.py
and tests/gpu/test_sample_report_gpu.py; inputs and bounds are tests/sample_cases.py.
"""
import re

import numpy as np
import pytest
import torch

from multidisttorch_amd.data.datasets import synthetic_images
from multidisttorch_amd.hpo import runner
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models import iw, latent
from multidisttorch_amd.models import sample_report as sr
from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from multidisttorch_amd.ops.philox import reparam_eps
from tests import sample_cases as sc

KEYS = {"rows_real", "rows_fake", "mean_pair_d2", "bandwidths", "mmd2", "mmd2_per_bandwidth", "nn_acc", "nn_acc_real",
        "nn_acc_fake", "nn_dist_real_to_fake", "nn_dist_fake_to_real", "rf_asym"}
SCALARS = ("mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake", "nn_dist_real_to_fake", "nn_dist_fake_to_real")


def _cloud(n, D, seed, shift=0.0):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) + shift


def test_stream_word_and_z_definition():
    assert sr.SAMPLE_STREAM == 5 << 28
    assert sr.SAMPLE_STREAM not in (iw.IW_STREAM, latent.LATENT_STREAM, 1 << 30)
    np.testing.assert_array_equal(sr.sample_z(7, 5, 11), reparam_eps(7, 5, 11, 5 << 28, 0))
    assert sr.BANDWIDTH_SCALES == (0.25, 1.0, 4.0) and sr.COLS == 8


def test_two_halves_of_one_cloud_are_not_told_apart():
    x = _cloud(400, 8, 1)
    r = sr.sample_report(x[:200], x[200:])
    assert set(r) == KEYS and r["rows_real"] == r["rows_fake"] == 200
    assert abs(r["mmd2"]) < 0.01 and 0.4 <= r["nn_acc"] <= 0.6
    assert r["bandwidths"] == [c * r["mean_pair_d2"] for c in sr.BANDWIDTH_SCALES]
    assert abs(r["mmd2"] - sum(r["mmd2_per_bandwidth"]) / 3) < 1e-15


def test_a_shifted_copy_is_told_apart():
    x = _cloud(200, 8, 2)
    r = sr.sample_report(x, _cloud(200, 8, 3, shift=3.0))
    assert r["mmd2"] > 0.1 and r["nn_acc"] > 0.95 and r["nn_acc_real"] > 0.95 and r["nn_acc_fake"] > 0.95


def test_mean_pair_d2_is_the_mean_over_real_pairs():
    x = _cloud(37, 5, 4)
    d2 = ((x[:, None] - x[None]) ** 2).sum(-1)
    assert abs(sr.mean_pair_d2(x) - float(d2.sum()) / (37 * 36)) < 1e-12 * float(d2.max())


def test_mmd_is_symmetric_under_fixed_bandwidths_and_rf_asym_is_zero():
    a, b = _cloud(60, 6, 5), _cloud(60, 6, 6, shift=0.5)
    h = sr.bandwidths_of(sr.mean_pair_d2(a))
    ab, ba = sr.sample_report(a, b, bandwidths=h), sr.sample_report(b, a, bandwidths=h)
    np.testing.assert_allclose(ab["mmd2_per_bandwidth"], ba["mmd2_per_bandwidth"], rtol=0, atol=1e-14)
    assert ab["rf_asym"] <= 1e-14 and ba["rf_asym"] <= 1e-14
    assert abs(ab["nn_dist_real_to_fake"] - ba["nn_dist_fake_to_real"]) < 1e-14
    assert sr.sample_report(b, a)["bandwidths"] != list(h)  # its own bandwidths: those of b's rows


def test_float32_oracle_agrees_with_float64():
    a, b = _cloud(80, 20, 7), _cloud(70, 20, 8, shift=0.3)
    r64, r32 = sr.sample_report(a, b), sr.sample_report(a.float(), b.float())
    assert abs(r32["mmd2"] - r64["mmd2"]) <= 1e-4 * abs(r64["mmd2"])
    assert r32["nn_acc"] == r64["nn_acc"]


def test_chunked_rows_match_unchunked():
    a, b = _cloud(23, 7, 9), _cloud(19, 7, 10)
    h = sr.bandwidths_of(sr.mean_pair_d2(a))
    np.testing.assert_allclose(sr.sample_rows(a, b, h, chunk=5).numpy(), sr.sample_rows(a, b, h).numpy(), rtol=1e-13)


def test_a_tie_counts_as_real():
    real, fake = sc.lattice(9, 7, 5, dup="fake")
    r = sr.sample_report(real.double(), fake.double(), return_rows=True)
    t = r["table"]
    assert float(t[9, 0]) == 0.0 and float(t[9, 1]) > 0.0      # the copy: nearest real at 0, and it counts as real
    assert float(t[1, 1]) == 0.0                                # the copied real row finds it at 0 ...
    real2 = torch.cat([real, real[1:2]])                        # ... and with a real twin as well: a tie, real
    t2 = sr.sample_report(real2.double(), fake.double(), return_rows=True)["table"]
    assert float(t2[1, 0]) == 0.0 == float(t2[1, 1])
    s = sr.sample_stats(t2, 10, 7)
    right = (t2[:10, 0] <= t2[:10, 1]).sum().item()
    assert s["nn_acc_real"] == right / 10 and bool(t2[1, 0] <= t2[1, 1])
    assert s["nn_acc_fake"] == (t2[10:, 0] > t2[10:, 1]).sum().item() / 7 and not bool(t2[10, 0] > t2[10, 1])


def test_argument_validation():
    x = _cloud(5, 3, 11)
    with pytest.raises(ValueError, match="real rows that differ"):
        sr.sample_report(torch.ones(4, 3), x)
    for na, nb, D, text in ((1, 5, 3, "got 1 real rows"), (5, 1, 3, "got 1 generated rows"),
                            (32769, 5, 3, "got 32769 real rows"), (5, 32769, 3, "got 32769 generated rows"),
                            (5, 5, 0, "got D = 0"), (5, 5, 65537, "got D = 65537")):
        with pytest.raises(ValueError, match=re.escape(text)):
            sr.check_sample_args(na, nb, D)
    sr.check_sample_args(2, 2, 1)
    sr.check_sample_args(32768, 32768, 65536)
    with pytest.raises(ValueError, match="differ in width"):
        sr.sample_rows(x, _cloud(5, 4, 12), (1.0, 2.0, 3.0))


# ---- evaluate_samples on both trainers, torch backend ----
N = 24


def _mlp(**kw):
    kw.setdefault("seed", 3)
    tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", lr=3e-3, **kw)
    X = torch.rand(64, 20, generator=torch.Generator().manual_seed(7))
    return tr, X


def _conv(**kw):
    kw.setdefault("seed", 3)
    tr = ConvVaeTrainer(batch_size=8, image=28, z=32, device="cpu", backend="torch", **kw)
    return tr, synthetic_images(32, seed=3)


def _train(tr, X, steps):
    tr.bind_train_data(X, torch.arange(X.shape[0], dtype=torch.int32))
    tr.set_cursor(0, X.shape[0] // tr.B)
    tr.train_steps(steps)


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_torch_backend_is_the_oracle_on_the_decoded_prior_draw(make):
    tr, X = make()
    _train(tr, X, 2)
    idx = torch.arange(N)
    r = tr.evaluate_samples(X, idx, 19, return_rows=True)
    assert set(r) == KEYS | {"table", "real", "fake"} and set(tr.evaluate_samples(X, idx)) == KEYS
    assert r["rows_real"] == N and r["rows_fake"] == 19 and tr.evaluate_samples(X, idx)["rows_fake"] == N
    z = torch.from_numpy(reparam_eps(19, tr.Z, 3, 5 << 28, 0))
    fake = tr.decode(z).reshape(19, -1)
    assert torch.equal(r["fake"], fake) and torch.equal(r["real"], X[:N].reshape(N, -1))
    o = sr.sample_report(X[:N].reshape(N, -1).double(), fake.double())
    assert r["nn_acc"] == o["nn_acc"] and r["nn_acc_real"] == o["nn_acc_real"]
    for k in ("mmd2", "nn_dist_real_to_fake", "nn_dist_fake_to_real", "mean_pair_d2"):
        assert abs(r[k] - o[k]) <= 1e-4 * max(abs(o[k]), 1e-3), (k, r[k], o[k])
    assert r["rf_asym"] < 1e-5


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_result_depends_on_weights_data_seed_and_n_only(make):
    idx = torch.arange(N)
    tr, X = make()
    base = tr.evaluate_samples(X, idx)
    r = make(rng_stream=3)[0].evaluate_samples(X, idx)
    assert all(r[k] == base[k] for k in KEYS)
    other = make(seed=4, init_seed=3)[0].evaluate_samples(X, idx)
    assert other["mean_pair_d2"] == base["mean_pair_d2"] and other["mmd2"] != base["mmd2"]  # the seed draws z


def _frozen(v):
    """A deep copy of a (nested) state: tensors and arrays cloned."""
    if torch.is_tensor(v):
        return v.clone()
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, dict):
        return {k: _frozen(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_frozen(x) for x in v)
    return v


def _assert_same(a, b, where):
    """Every leaf of a nested state, bitwise."""
    assert type(a) is type(b), where
    if torch.is_tensor(a):
        assert torch.equal(a, b), where
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b, err_msg=where)
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _assert_same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, f"{where}[{i}]")
    else:
        assert a == b or (a != a and b != b), where


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_pass_leaves_the_trainer_alone(make):
    tr, X = make()
    _train(tr, X, 2)
    tr.evaluate(X, torch.arange(N), want_first_recon=False)
    sd = _frozen(tr.state_dict())
    before = (tr.read_state(), tr.read_state(eval=True), tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
    tr.evaluate_samples(X, torch.arange(N))
    assert tr.read_state() == before[0] and tr.read_state(eval=True) == before[1]
    assert torch.equal(tr.params, before[2]) and torch.equal(tr.exp_avg, before[3]) and torch.equal(tr.exp_avg_sq, before[4])
    _assert_same(tr.state_dict(), sd, "state_dict")


def test_domain_is_checked_before_any_work():
    tr, X = _mlp()
    with pytest.raises(ValueError, match="got 1 real rows"):
        tr.evaluate_samples(X, torch.arange(1))
    with pytest.raises(ValueError, match="got 1 generated rows"):
        tr.evaluate_samples(X, torch.arange(N), 1)
    with pytest.raises(ValueError, match="real rows that differ"):
        tr.evaluate_samples(torch.ones(8, 20), torch.arange(8))


class _Metrics:
    def __init__(self):
        self.rows = []

    def log(self, **kw):
        self.rows.append(kw)


class _Test:
    def __init__(self, X):
        self.data = X

    def __len__(self):
        return self.data.shape[0]


def test_runner_pass_uses_the_averaged_weights(capsys):
    tr, X = _mlp(ema_decay=0.5)
    _train(tr, X, 4)
    opts = runner.RunOptions(sample_report=N)
    m = _Metrics()
    out = runner._sample_eval(tr, _Test(X), opts, None, m, torch.device("cpu"))
    r = out["sample_report"]
    with tr.averaged_weights():
        avg = tr.evaluate_samples(X, torch.arange(N), N)
    raw = tr.evaluate_samples(X, torch.arange(N), N)
    assert all(r[k] == avg[k] for k in KEYS) and raw["mmd2"] != avg["mmd2"]
    assert r["sample_s"] > 0 and m.rows == [dict(event="sample_eval", **r)]
    line = capsys.readouterr().out.strip()
    assert "\n" not in line and line.endswith(  # print0 puts the rank in front
        "====> Test set samples: MMD2 {:.6f} 1-NN acc {:.4f} (real {:.4f} gen {:.4f})".format(
            r["mmd2"], r["nn_acc"], r["nn_acc_real"], r["nn_acc_fake"]))
    with pytest.raises(ValueError, match="exceeds the test set's 64 rows"):
        runner._sample_eval(tr, _Test(X), runner.RunOptions(sample_report=65), None, m, torch.device("cpu"))


def test_after_trial_table_and_options():
    assert [row[0] for row in runner._AFTER_TRIAL][-1] == "sample pass"
    assert runner._AFTER_TRIAL[-1][2] is runner._sample_eval
    spec = build_specs(1, 1)[0]
    enabled = runner._AFTER_TRIAL[-1][1]
    assert not enabled(spec, runner.RunOptions()) and enabled(spec, runner.RunOptions(sample_report=2))
    import dataclasses

    # the count is checked against the test set when a trial starts, before any training
    runner._check_sample_rows(runner.RunOptions(sample_report=64), _Test(torch.zeros(64, 4)))
    runner._check_sample_rows(runner.RunOptions(), _Test(torch.zeros(0, 4)))
    with pytest.raises(ValueError, match="--sample-report 65 exceeds the test set's 64 rows"):
        runner._check_sample_rows(runner.RunOptions(sample_report=65), _Test(torch.zeros(64, 4)))
    f = dataclasses.fields(runner.RunOptions)[-1]
    assert f.name == "sample_report" and f.default == 0
