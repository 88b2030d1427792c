"""The k-means kernels behind ``--ndb`` (csrc/kernels/kmeans.hip) against the float64 oracle (models/ndb.py) on
inputs the oracle decides by a margin (tests/ndb_cases.py): the two steps alone, the whole fit, the fit through
both trainers, and the domain."""
import pytest
import torch

from multidisttorch_amd.models import ndb
from tests import ndb_cases as nc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _ws(C, na, nb, D, K):
    return torch.empty(C.kmeans_ws_numel(na, nb, D, K), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("n,D,K", nc.ASSIGN)
def test_assign_step(n, D, K, native_ext):
    C, c = native_ext, nc.assign_case(n, D, K)
    x, cent = c["x"].to(DEV), c["cent"].to(DEV)
    labels, mind, moved = C.kmeans_assign(x, None, cent, _ws(C, n, 0, D, K), c["prev"].to(DEV))
    nc.report(f"assign {n}x{D} K={K} band {C.kmeans_layout(n)['band']}",
              mind=float((mind.double().cpu() - c["mind"]).abs().max()) / c["bound"])
    assert torch.equal(labels.cpu().long(), c["labels"]) and int(moved) == c["moved"]
    assert int(C.kmeans_assign(x, None, cent, _ws(C, n, 0, D, K))[2]) == n  # no previous labels: every row counts


@pytest.mark.parametrize("n,D,K", nc.UPDATE)
def test_update_step(n, D, K, native_ext):
    C, c = native_ext, nc.update_case(n, D, K)
    cent, counts = C.kmeans_update(c["x"].to(DEV), c["labels"].to(DEV), c["cent_in"].to(DEV), _ws(C, n, 0, D, K))
    cent = cent.cpu()
    nc.report(f"update {n}x{D} K={K}", centroids=float((cent.double() - c["cent"]).abs().max()) / c["bound"])
    assert torch.equal(counts.cpu().long(), c["counts"]) and bool(c["empty"].any())
    assert torch.equal(cent[c["empty"]], c["cent_in"][c["empty"]])  # bit for bit


@pytest.mark.parametrize("kind,na,nb,D,K", nc.FIT)
def test_whole_fit(kind, na, nb, D, K, native_ext):
    C, c = native_ext, nc.fit_case(kind, na, nb, D, K)
    run = lambda: C.kmeans_rows(c["real"].to(DEV), c["fake"].to(DEV), K, nc.T_FIT, c["init"].to(DEV), _ws(C, na, nb, D, K))
    first, second = run(), run()
    labels, mind, cent, moved, inertia = first
    assert torch.equal(labels.cpu().long(), c["labels"]) and moved.tolist() == c["moved"]
    nc.check_stats(ndb.ndb_stats(labels, na, K, float(inertia), int(moved[-1]), nc.T_FIT), c, f"fit {kind}")
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def _trainer(kind):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    X = synthetic_images(128, size=28, seed=5, device=DEV)
    if kind == "mlp":
        tr = MlpVaeTrainer(batch_size=16, device=DEV, backend="hip", seed=7, use_graphs=False)
    else:
        tr = ConvVaeTrainer(batch_size=16, image=28, z=32, device=DEV, backend="hip", seed=7, use_graphs=False)
    tr.bind_train_data(X, torch.arange(128, dtype=torch.int32, device=DEV))
    tr.set_cursor(0, 4)
    tr.train_steps(3)
    torch.cuda.synchronize()
    return tr, X, torch.arange(50, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_through_the_trainers(kind, native_ext):
    tr, X, idx = _trainer(kind)
    base = tr.evaluate_samples(X, idx, 64, return_rows=True)
    r = tr.evaluate_samples(X, idx, 64, return_rows=True, ndb=4, ndb_iters=5, ndb_group=2)
    assert set(r) == set(base) | {"ndb", "ndb_labels", "ndb_centroids"} and torch.equal(r["table"], base["table"])
    c = nc.reference(r["real"].cpu(), r["fake"].cpu(), ndb.ndb_init_idx(50, 4, 7, 2), 4, 5)
    assert torch.equal(r["ndb_labels"].cpu().long(), c["labels"])
    nc.check_stats(r["ndb"], c, kind)
    g = tr.evaluate_samples(X, idx, 64, return_rows=True, ndb=4, ndb_iters=5, ndb_group=2, gmm_k=2, gmm_iters=5,
                            fit_rows=(X, torch.arange(128)))
    cg = nc.decide(torch.cat([g["real"], g["gmm_fake"]]).cpu(), g["ndb_centroids"].cpu())[0]
    want = ndb.ndb_stats(cg, 50, 4, r["ndb"]["inertia"], r["ndb"]["moved"], 5)
    assert g["gmm"]["ndb"] == want and g["ndb"] == r["ndb"] and "ndb" not in g["gmm"]["sample_report"]


@pytest.mark.parametrize("na,D,K,T", [(40, 8, 1, 5), (300, 8, 257, 5), (40, 8, 41, 5), (40, 8, 4, 0), (40, 0, 4, 5)])
def test_domain_errors(na, D, K, T, native_ext):
    C = native_ext
    real, fake = torch.zeros(na, D, device=DEV), torch.zeros(40, D, device=DEV)
    init = torch.arange(K, device=DEV)
    with pytest.raises(ValueError):
        C.kmeans_check(na, 40, D, K, T)
    with pytest.raises(ValueError):
        C.kmeans_rows(real, fake, K, T, init, torch.empty(16, device=DEV))
