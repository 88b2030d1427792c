"""``evaluate_recon(return_rows=True)`` on the HIP backends of both trainers, eager
and with graphs, over a ragged row count: ``mu`` is the latent pass's, ``recon``
the decoder's, the table the oracle's on the returned rows within the kernels'
bounds (tests/recon_cases.py); the latent report, the training state, the eval
state and a following training step are what they are without the pass."""
import numpy as np
import pytest
import torch

from multidisttorch_amd.models import recon_report as rr
from tests import recon_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

KINDS = ["mlp", "conv28-fused", "conv28-layers", "conv128"]


def _make(kind, graphs, monkeypatch):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    size, B = (128, 8) if kind == "conv128" else (28, 16)
    X = synthetic_images(4 * B, size=size, seed=5, device=DEV)
    kw = dict(batch_size=B, device=DEV, backend="hip", seed=7, use_graphs=graphs, graph_steps=2)
    if kind == "mlp":
        tr = MlpVaeTrainer(**kw)
    else:
        monkeypatch.setenv("MDT_CONV_F28", "0" if kind == "conv28-layers" else "1")
        tr = ConvVaeTrainer(image=size, z=32 if size == 28 else 64, **kw)
        assert tr.f28 == (kind == "conv28-fused")
    tr.bind_train_data(X, torch.arange(4 * B, dtype=torch.int32, device=DEV))
    tr.set_cursor(0, 4)
    tr.train_steps(2)
    torch.cuda.synchronize()
    return tr, X, torch.arange(2 * B + 5, dtype=torch.int32, device=DEV)   # two batches and a ragged tail


def _state(tr):
    return ([t.clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)], tr.read_state(), tr.read_state(eval=True),
            tr.loss_history().copy(), tr.loss_history(eval=True).copy())


def _same(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1:3] == b[1:3]
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[4], b[4])


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("kind", KINDS)
def test_pass_is_the_oracle_on_its_own_rows_and_touches_nothing(kind, graphs, native_ext, monkeypatch):
    tr, X, idx = _make(kind, graphs, monkeypatch)
    n, Z, S = idx.numel(), tr.Z, 128 if kind == "conv128" else 28
    tr.evaluate(X, idx, want_first_recon=False)
    lat = tr.evaluate_latent(X, idx, return_rows=True)
    mulv = tr.latent_buffers()["mulv"]
    before = _state(tr)
    r = tr.evaluate_recon(X, idx, return_rows=True)
    assert set(tr.evaluate_recon(X, idx)) == set(r) - {"table", "real", "recon", "mu"}
    _same(before, _state(tr))
    with pytest.raises(RuntimeError, match="no evaluate_latent pass"):
        tr.latent_buffers()
    assert torch.equal(r["mu"], mulv[:, :Z]) and torch.equal(r["recon"], tr.decode(r["mu"]))
    assert torch.equal(r["real"], X[idx.long()].float()) and r["table"].shape == (n, rr.COLS)
    real, recon = r["real"].cpu(), r["recon"].cpu()
    o64, bound = rc.bounds(real, recon, S)
    rc.check(r["table"], o64, bound, f"{kind} {'graphs' if graphs else 'eager'}")
    assert {k: r[k] for k in rr.recon_stats(r["table"], S)} == rr.recon_stats(r["table"], S) and r["rows"] == n
    again = tr.evaluate_latent(X, idx, return_rows=True)
    assert all(torch.equal(v, again[k]) if torch.is_tensor(v) else v == again[k] for k, v in lat.items())
    assert torch.equal(tr.latent_buffers()["mulv"], mulv)
    # a following training step: the same as on a trainer that never ran the pass
    ref, _, _ = _make(kind, graphs, monkeypatch)
    for t in (tr, ref):
        t.set_cursor(0, 4)
        t.train_steps(2)
    torch.cuda.synchronize()
    assert torch.equal(tr.params, ref.params) and torch.equal(tr.exp_avg_sq, ref.exp_avg_sq)
    assert tr.read_state() == ref.read_state()
