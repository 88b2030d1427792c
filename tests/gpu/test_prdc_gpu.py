"""``evaluate_samples(prdc_k=5)`` on the HIP backends of both trainers against the
float64 oracle (models/prdc.py) applied to the returned ``real`` and ``fake``
rows on the CPU: rad and dminx within the kernels' bounds for float inputs, the
four statistics inside what the count intervals admit (tests/prdc_cases.py).
The default call and the training state are what they were."""
import numpy as np
import pytest
import torch

from multidisttorch_amd.models import prdc
from tests import prdc_cases as pc

pytestmark = pytest.mark.gpu

SEED, K = 7, 5


def _dev():
    return torch.device("cuda", 0)


def _make(kind):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    size, B, n = (128, 8, 24) if kind == "conv128" else (28, 16, 50)   # n is no multiple of B
    X = synthetic_images(64 if size == 28 else 32, size=size, seed=5, device=_dev())
    if kind == "mlp":
        tr = MlpVaeTrainer(batch_size=B, device=_dev(), backend="hip", seed=SEED, use_graphs=False)
    else:
        tr = ConvVaeTrainer(batch_size=B, image=size, z=32 if size == 28 else 64, device=_dev(), backend="hip",
                            seed=SEED, use_graphs=False)
    m = X.shape[0] // B * B
    tr.bind_train_data(X, torch.arange(m, dtype=torch.int32, device=_dev()))
    tr.set_cursor(0, m // B)
    tr.train_steps(3)
    torch.cuda.synchronize()
    return tr, X, torch.arange(n, dtype=torch.int32, device=_dev()), n


@pytest.mark.parametrize("kind", ["mlp", "conv28", "conv128"])
def test_statistics_match_the_oracle_on_the_trainers_own_samples(kind, native_ext):
    tr, X, idx, n = _make(kind)
    base = tr.evaluate_samples(X, idx, n, return_rows=True)
    r = tr.evaluate_samples(X, idx, n, return_rows=True, prdc_k=K)
    assert set(r) == set(base) | {"prdc", "prdc_table"} and set(tr.evaluate_samples(X, idx, n)) == set(base) - {
        "table", "real", "fake"}
    assert torch.equal(r["real"], base["real"]) and torch.equal(r["fake"], base["fake"])
    assert torch.equal(r["table"], base["table"])                                        # the default table, bitwise
    assert torch.equal(tr.evaluate_samples(X, idx, n, return_rows=True)["table"], base["table"])   # and after the pass
    real, fake, got = r["real"].cpu(), r["fake"].cpu(), r["prdc_table"].cpu().double()
    D = real.shape[1]
    table = prdc.prdc_rows(real.double(), fake.double(), K, chunk=max(1, (1 << 22) // (n * D)))
    b = pc.float_bounds(real, fake)
    for c, name in ((0, "rad"), (2, "dminx")):
        err = (got[:, c] - table[:, c]).abs()
        print(f"{kind} {name}: max error/bound {float((err / b[name]).max()):.3f} (max error {float(err.max()):.3e})")
        assert bool((err <= b[name]).all()), name
    o = prdc.prdc_stats(table, n, n, K)
    assert list(r["prdc"]) == list(o) and r["prdc"]["k"] == K
    for name, (lo, hi) in pc.stat_interval(table, n, n, K, b).items():
        print(f"{kind} {name}: {r['prdc'][name]:.6f} oracle {o[name]:.6f} admissible [{lo:.6f}, {hi:.6f}]")
        assert lo - 1e-12 <= r["prdc"][name] <= hi + 1e-12, name


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_pass_leaves_params_adam_train_and_eval_state_bitwise(kind, native_ext):
    tr, X, idx, n = _make(kind)
    tr.evaluate(X, idx, want_first_recon=False)
    before = [t.clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]
    st = (tr.read_state(), tr.read_state(eval=True), tr.loss_history().copy(), tr.loss_history(eval=True).copy())
    tr.evaluate_samples(X, idx, prdc_k=K)
    torch.cuda.synchronize()
    for a, t in zip(before, (tr.params, tr.exp_avg, tr.exp_avg_sq)):
        assert torch.equal(a, t)
    assert tr.read_state() == st[0] and tr.read_state(eval=True) == st[1]
    np.testing.assert_array_equal(tr.loss_history(), st[2])
    np.testing.assert_array_equal(tr.loss_history(eval=True), st[3])
