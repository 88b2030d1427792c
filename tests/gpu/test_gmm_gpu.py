"""``C.gmm_fit`` against the float64 oracle's fit (models/gmm.py, on the CPU), and ``evaluate_samples(gmm_k=)`` on
the HIP backends of both trainers against the oracle applied to the pass's own codes; tolerances by the rule of
tests/gmm_cases.py. The call without ``gmm_k`` is what it was."""
import pytest
import torch

from multidisttorch_amd.models import gmm
from tests import gmm_cases as gc

pytestmark = pytest.mark.gpu

SEED, T = 7, 20


def _fit(C, z, K, iters):
    n, Z = z.shape
    flat = torch.full((K * (1 + Z + Z * Z),), float("nan"), dtype=torch.float32, device=z.device)
    hist = torch.full((iters + 1,), float("nan"), dtype=torch.float32, device=z.device)
    C.gmm_fit(z, K, iters, torch.full((C.gmm_ws_numel(n, Z, K),), float("nan"), device=z.device), flat, hist)
    return flat.cpu(), hist.cpu()


@pytest.mark.parametrize("shape", [(5000, 32, 10), (130, 20, 10)], ids=["5000x32x10", "130x20x10"])
def test_fit_follows_the_oracles_history_and_repeats_bitwise(shape, native_ext):
    from multidisttorch_amd.ops import native

    (n, Z, K), z = shape, gc.planted(*shape)[0]
    ref64, ref32 = gmm.gmm_fit(z.double(), K, T)["ll_history"], gmm.gmm_fit(z, K, T)["ll_history"]
    a, b = (_fit(native.require(), z.to("cuda:0"), K, T) for _ in range(2))
    err, tol = float((a[1].double() - ref64).abs().max()), gc.tolerance(ref64, ref32)
    print(f"{shape}: ll_history max error {err:.3e}, tolerance {tol:.3e}; {a[1][0]:.5f} -> {a[1][-1]:.5f}")
    assert err <= tol
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])   # no float atomics anywhere


def _make(kind):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    dev, B = torch.device("cuda", 0), 16
    X = synthetic_images(256, size=28, seed=5, device=dev)
    if kind == "mlp":
        tr = MlpVaeTrainer(batch_size=B, device=dev, backend="hip", seed=SEED, use_graphs=False)
    else:
        tr = ConvVaeTrainer(batch_size=B, image=28, z=32, device=dev, backend="hip", seed=SEED, use_graphs=False)
    tr.bind_train_data(X, torch.arange(256, dtype=torch.int32, device=dev))
    tr.set_cursor(0, 4)
    tr.train_steps(3)
    torch.cuda.synchronize()
    return tr, X, torch.arange(64, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_trainer_report_matches_the_oracle_on_its_own_codes(kind, native_ext):
    """The mean of per-row values errs by at most the largest per-row error, so the rule is applied to the rows."""
    tr, X, idx = _make(kind)
    base = tr.evaluate_samples(X, idx, 64, return_rows=True)
    r = tr.evaluate_samples(X, idx, 64, return_rows=True, gmm_k=3, gmm_iters=10, fit_rows=(X, torch.arange(256)))
    assert set(r) == set(base) | {"gmm", "gmm_params", "gmm_fake", "gmm_fit_z", "gmm_test_z"}
    for k, v in base.items():   # every other entry, bitwise
        assert torch.equal(r[k], v) if torch.is_tensor(v) else r[k] == v, k
    zf, zt, g = r["gmm_fit_z"].cpu(), r["gmm_test_z"].cpu(), r["gmm"]
    assert zf.shape == (256, tr.Z) and zt.shape == (64, tr.Z) and r["gmm_fake"].shape == r["fake"].shape
    ll64, ll32 = gmm.gmm_score(zt.double(), gmm.gmm_fit(zf.double(), 3, 10)), gmm.gmm_score(zt, gmm.gmm_fit(zf, 3, 10))
    lp64, lp32 = gmm.prior_score(zt.double()), gmm.prior_score(zt)
    tl, tp = gc.tolerance(ll64, ll32), gc.tolerance(lp64, lp32)
    el, ep = abs(g["ll_test"] - float(ll64.mean())), abs(g["lp_test"] - float(lp64.mean()))
    print(f"{kind}: ll_test error {el:.3e} tolerance {tl:.3e}, lp_test error {ep:.3e} tolerance {tp:.3e}; "
          f"{ {k: v for k, v in g.items() if k not in ('ll_history', 'sample_report')} }")
    assert el <= tl and ep <= tp and abs(g["gap"] - float(ll64.mean() - lp64.mean())) <= tl + tp
    assert (g["k"], g["iters"], g["rows_fit"], len(g["ll_history"])) == (3, 10, 256, 11) and g["ll_fit"] == g["ll_history"][-1]
    assert set(g["sample_report"]) == set(base) - {"table", "real", "fake"}
