"""``evaluate_samples(sinkhorn_blur=E)`` on the HIP backends of both trainers against the float64 oracle
(models/sinkhorn.py) applied to the returned ``real`` and ``fake`` rows on the CPU, within the bounds for float
inputs (tests/sinkhorn_cases.py). The mixture's draws get the distance too; the call without it is what it was."""
import pytest
import torch

from tests import sinkhorn_cases as kc

pytestmark = pytest.mark.gpu

SEED, E, T = 7, 0.05, 12


def _make(kind):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    dev, B = torch.device("cuda", 0), 16
    X = synthetic_images(128, size=28, seed=5, device=dev)
    if kind == "mlp":
        tr = MlpVaeTrainer(batch_size=B, device=dev, backend="hip", seed=SEED, use_graphs=False)
    else:
        tr = ConvVaeTrainer(batch_size=B, image=28, z=32, device=dev, backend="hip", seed=SEED, use_graphs=False)
    tr.bind_train_data(X, torch.arange(128, dtype=torch.int32, device=dev))
    tr.set_cursor(0, 4)
    tr.train_steps(3)
    torch.cuda.synchronize()
    return tr, X, torch.arange(50, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_distance_matches_the_oracle_on_the_trainers_own_samples(kind, native_ext):
    tr, X, idx = _make(kind)
    base = tr.evaluate_samples(X, idx, 64, return_rows=True)
    off = tr.evaluate_samples(X, idx, 64, return_rows=True, sinkhorn_blur=0.0)
    r = tr.evaluate_samples(X, idx, 64, return_rows=True, sinkhorn_blur=E, sinkhorn_iters=T)
    assert set(off) == set(base) and set(r) == set(base) | {"sinkhorn", "sinkhorn_pot"}
    for k, v in base.items():   # every other entry, bitwise, with the blur at 0 and with it set
        for other in (off, r):
            assert torch.equal(other[k], v) if torch.is_tensor(v) else other[k] == v, k
    case = kc.reference(r["real"].cpu(), r["fake"].cpu(), E, T, exact_costs=False)
    s = r["sinkhorn"]
    assert r["sinkhorn_pot"].shape == (114, 2) and list(s) == ["blur", "iters", "scale", "sinkhorn", "w2", "ot", "marg_err"]
    assert kc.check(r["sinkhorn_pot"], s["scale"], s["marg_err"], case, E, T, kind) == s
    g = tr.evaluate_samples(X, idx, 64, sinkhorn_blur=E, sinkhorn_iters=T, gmm_k=2, gmm_iters=5,
                            fit_rows=(X, torch.arange(128)))["gmm"]
    assert g["sinkhorn"]["iters"] == T and g["sinkhorn"]["scale"] == s["scale"] and "sinkhorn" not in g["sample_report"]
