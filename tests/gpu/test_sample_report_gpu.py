"""``evaluate_samples`` on the HIP backends of both trainers against the float64
oracle (models/sample_report.py) applied to the trainer's own ``decode(z)``
output copied to the CPU. The bounds are the kernels' per-row bounds for float
inputs (tests/sample_cases.py) propagated to each statistic: sums of the row
bounds for the MMD terms, rows whose oracle gap is inside the distance bound
left open for the accuracies, bound / sqrt(d2) for the mean distances. Each
check prints the achieved error next to its bound.
"""
import numpy as np
import pytest
import torch

from multidisttorch_amd.models import sample_report as sr
from tests import sample_cases as sc

pytestmark = pytest.mark.gpu

SEED, B, N = 7, 16, 50   # N is no multiple of B: the decoder's last chunk is partial
KEYS = {"rows_real", "rows_fake", "mean_pair_d2", "bandwidths", "mmd2", "mmd2_per_bandwidth", "nn_acc", "nn_acc_real",
        "nn_acc_fake", "nn_dist_real_to_fake", "nn_dist_fake_to_real", "rf_asym"}


def _dev():
    return torch.device("cuda", 0)


def _images(n=64):
    from multidisttorch_amd.data.datasets import synthetic_images

    return synthetic_images(n, size=28, seed=5, device=_dev())


def _mlp(**kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    return MlpVaeTrainer(batch_size=B, device=_dev(), backend="hip", seed=SEED, use_graphs=False, **kw)


def _conv(**kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    return ConvVaeTrainer(batch_size=B, image=28, z=32, device=_dev(), backend="hip", seed=SEED, use_graphs=False, **kw)


def _train(tr, X, steps):
    n = X.shape[0] // tr.B * tr.B
    tr.bind_train_data(X, torch.arange(n, dtype=torch.int32, device=X.device))
    tr.set_cursor(0, n // tr.B)
    tr.train_steps(steps)
    torch.cuda.synchronize()


def _idx(n=N):
    return torch.arange(n, dtype=torch.int32, device=_dev())


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_statistics_match_the_oracle_on_the_trainers_own_samples(make, native_ext):
    from multidisttorch_amd.ops.philox import reparam_eps

    X = _images()
    tr = make()
    _train(tr, X, 3)
    r = tr.evaluate_samples(X, _idx(), return_rows=True)
    assert set(r) == KEYS | {"table", "real", "fake"} and set(tr.evaluate_samples(X, _idx())) == KEYS
    assert r["rows_real"] == N and r["rows_fake"] == N and r["table"].shape == (2 * N, 8)
    z = torch.from_numpy(reparam_eps(N, tr.Z, SEED, 5 << 28, 0))
    assert torch.equal(r["fake"], tr.decode(z).reshape(N, -1)) and torch.equal(r["real"], X[:N].reshape(N, -1))
    real, fake = r["real"].cpu(), r["fake"].cpu()
    m = sr.mean_pair_d2(real)
    assert abs(r["mean_pair_d2"] - m) <= 1e-12 * m and r["bandwidths"] == list(sr.bandwidths_of(r["mean_pair_d2"]))
    h = r["bandwidths"]
    table = sc.oracle_table(real, fake, h)
    o = sr.sample_stats(table, N, N)
    dmin_b, ksum_b = sc.float_bounds(real, fake, h, table)
    b = sc.stat_bounds(table, dmin_b, ksum_b, N, N)
    name = type(tr).__name__
    for k in ("mmd2", "nn_dist_real_to_fake", "nn_dist_fake_to_real"):
        print(f"{name} {k}: {r[k]:.9g} oracle {o[k]:.9g} error {abs(r[k] - o[k]):.3e} bound {b[k]:.3e}")
        assert abs(r[k] - o[k]) <= b[k], k
    err = np.abs(np.array(r["mmd2_per_bandwidth"]) - np.array(o["mmd2_per_bandwidth"]))
    assert (err <= b["mmd2_per_bandwidth"].numpy()).all(), (err, b["mmd2_per_bandwidth"])
    for k in ("nn_acc", "nn_acc_real", "nn_acc_fake"):
        lo, hi = b[k]
        print(f"{name} {k}: {r[k]:.6f} oracle {o[k]:.6f} admissible [{lo:.6f}, {hi:.6f}]")
        assert lo - 1e-12 <= r[k] <= hi + 1e-12, k
    print(f"{name} rf_asym: {r['rf_asym']:.3e} bound {b['rf_asym']:.3e}")
    assert r["rf_asym"] <= b["rf_asym"]
    # a second sample count, and the result repeats
    r2 = tr.evaluate_samples(X, _idx(), 19)
    assert r2["rows_fake"] == 19 and r2["mean_pair_d2"] == r["mean_pair_d2"]
    again = tr.evaluate_samples(X, _idx())
    assert all(again[k] == r[k] for k in KEYS)


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_pass_leaves_params_adam_train_and_eval_state_bitwise(make, native_ext):
    X = _images()
    tr = make()
    _train(tr, X, 3)
    tr.evaluate(X, _idx(), want_first_recon=False)
    before = [t.clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]
    st = (tr.read_state(), tr.read_state(eval=True), tr.loss_history().copy(), tr.loss_history(eval=True).copy())
    tr.evaluate_samples(X, _idx())
    torch.cuda.synchronize()
    for a, t in zip(before, (tr.params, tr.exp_avg, tr.exp_avg_sq)):
        assert torch.equal(a, t)
    assert tr.read_state() == st[0] and tr.read_state(eval=True) == st[1]
    np.testing.assert_array_equal(tr.loss_history(), st[2])
    np.testing.assert_array_equal(tr.loss_history(eval=True), st[3])


@pytest.mark.parametrize("make", [_mlp, _conv], ids=["mlp", "conv"])
def test_averaged_weights_give_other_samples(make, native_ext):
    X = _images()
    tr = make(ema_decay=0.5)
    _train(tr, X, 4)
    raw = tr.evaluate_samples(X, _idx())
    with tr.averaged_weights():
        avg = tr.evaluate_samples(X, _idx())
    assert raw["mean_pair_d2"] == avg["mean_pair_d2"] and raw["mmd2"] != avg["mmd2"]
    assert tr.evaluate_samples(X, _idx())["mmd2"] == raw["mmd2"]


def test_domain_is_checked_before_any_work(native_ext):
    X = _images()
    tr = _mlp()
    with pytest.raises(ValueError, match="got 1 real rows"):
        tr.evaluate_samples(X, _idx(1))
    with pytest.raises(ValueError, match="got 1 generated rows"):
        tr.evaluate_samples(X, _idx(), 1)
