"""``evaluate_samples(swd_dirs=P)`` on the HIP backends of both trainers against the float64 oracle
(models/swd.py) applied to the returned ``real`` and ``fake`` rows on the CPU, within the bounds for float
inputs (tests/swd_cases.py). The call without it is what it was."""
import pytest
import torch

from multidisttorch_amd.models import swd
from tests import swd_cases as wc

pytestmark = pytest.mark.gpu

SEED, P = 7, 9


def _make(kind):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    dev, B = torch.device("cuda", 0), 16
    X = synthetic_images(64, size=28, seed=5, device=dev)
    if kind == "mlp":
        tr = MlpVaeTrainer(batch_size=B, device=dev, backend="hip", seed=SEED, use_graphs=False)
    else:
        tr = ConvVaeTrainer(batch_size=B, image=28, z=32, device=dev, backend="hip", seed=SEED, use_graphs=False)
    tr.bind_train_data(X, torch.arange(64, dtype=torch.int32, device=dev))
    tr.set_cursor(0, 4)
    tr.train_steps(3)
    torch.cuda.synchronize()
    return tr, X, torch.arange(50, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_table_matches_the_oracle_on_the_trainers_own_samples(kind, native_ext):
    tr, X, idx = _make(kind)
    base = tr.evaluate_samples(X, idx, 41, return_rows=True)
    r = tr.evaluate_samples(X, idx, 41, return_rows=True, swd_dirs=P)
    assert set(r) == set(base) | {"swd", "swd_table", "swd_proj"} and "swd" not in tr.evaluate_samples(X, idx, 41)
    for k, v in base.items():   # every other entry, bitwise
        assert torch.equal(r[k], v) if torch.is_tensor(v) else r[k] == v, k
    real, fake = r["real"].cpu(), r["fake"].cpu()
    dirs = torch.from_numpy(swd.swd_directions(P, real.shape[1], SEED))
    proj, table = swd.swd_rows(real.double(), fake.double(), dirs.double())
    pb, tb = wc.float_bounds(real, fake, dirs, table)
    perr, terr = (r["swd_proj"].cpu().double() - proj).abs(), (r["swd_table"].cpu().double() - table).abs()
    print(f"{kind}: proj max error/bound {float((perr / pb).max()):.3f}, table {float((terr / tb).max()):.3f}; {r['swd']}")
    assert r["swd_proj"].shape == (P, 91) and bool((perr <= pb).all()) and bool((terr <= tb).all())
    assert r["swd"] == swd.swd_stats(r["swd_table"]) and r["swd"]["dirs"] == P
