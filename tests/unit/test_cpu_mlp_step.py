"""The native CPU step (``MlpCpuStep``, csrc/runtime/cpu_mlp.cpp: what
``backend="torch"`` runs on a CPU host) against the float64 oracle
``reference_step`` + ``reference_adam_``, at the default shape and at ragged,
tiny, wide and non-multiple-of-4 ones.

Bounds (the project's): gradients ``max|got - ref| / max|ref| < 2e-4``
(test_forward_backward_matches_reference), Adam rtol 1e-5 / atol 1e-6
(test_adam_matches_torch), loss relative 1e-4.
"""

import math

import numpy as np
import pytest
import torch

from multidisttorch_amd.ops import native

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")

EVAL_STREAM = 1 << 30
WD = 0.01
# (B, M, D, H, Z); the CPU step has no multiple-of-4 limit
SHAPES = [(128, 128, 784, 400, 20), (48, 37, 100, 36, 12), (16, 5, 20, 20, 4), (32, 17, 256, 512, 32),
          (200, 200, 784, 400, 20), (7, 7, 10, 6, 3)]


def _trainer(B, D, H, Z, beta, seed=3, decoupled=False):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    tr = MlpVaeTrainer(batch_size=B, D=D, H=H, Z=Z, device="cpu", backend="torch", seed=seed, kl_beta=beta,
                       weight_decay=WD, decoupled_wd=decoupled, lr=2e-3)
    assert tr._cpu_native() is not None, "the torch backend on a CPU host must run the native step"
    return tr


def _data(B, D, seed=3):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(3 * B + 5, D, generator=g)
    idx = torch.randperm(X.shape[0], generator=g)[: 2 * B].to(torch.int32)
    return X, idx


@pytest.mark.parametrize("beta,decoupled", [(0.5, False), (1.0, True), (4.0, False)])
@pytest.mark.parametrize("B,M,D,H,Z", SHAPES)
def test_train_step_matches_float64_oracle(B, M, D, H, Z, beta, decoupled):
    from multidisttorch_amd.models.mlp_vae import reference_adam_, reference_step, views
    from multidisttorch_amd.ops.philox import reparam_eps

    tr = _trainer(B, D, H, Z, beta, decoupled=decoupled)
    X, idx = _data(B, D)
    tr.bind_train_data(X, idx)
    tr.set_cursor(1, 2)  # the second batch: rows idx[B : B + M]
    # non-trivial optimizer state as two earlier steps could have left it (v >= m^2, so the update stays of
    # the size of lr), on the tensors only: the padding stays zero
    used = torch.zeros(tr.numel, dtype=torch.bool)
    for _, o, s in tr.layout:
        used[o: o + math.prod(s)] = True
    g = torch.Generator().manual_seed(11)
    tr.exp_avg.copy_((torch.rand(tr.numel, generator=g) - 0.5) * 1e-2 * used)
    tr.exp_avg_sq.copy_((tr.exp_avg ** 2 + torch.rand(tr.numel, generator=g) * 1e-4) * used)
    tr.set_step(2)
    p = tr.params.clone().double()
    m, v2 = tr.exp_avg.clone().double(), tr.exp_avg_sq.clone().double()

    tr.train_steps(1, M)

    gr = torch.zeros_like(p)
    x = X[idx[B: B + M].long()].double()
    eps = torch.from_numpy(reparam_eps(M, Z, tr.seed, tr.rng_stream, 2)).double()
    f = reference_step(views(p, tr.layout), views(gr, tr.layout), x, eps, beta)
    worst = 0.0
    for name, ref in views(gr, tr.layout).items():
        got = tr.named_grads()[name].double()
        err = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
        worst = max(worst, err)
        assert err < 2e-4, (name, err)
    loss = float(tr.loss_history()[2])
    assert math.isclose(loss, float(f["loss"]), rel_tol=1e-4), (loss, float(f["loss"]))
    # Adam on the step's own gradients, so only the update is compared
    reference_adam_(p, tr.grads.double(), m, v2, 3, 2e-3, 0.9, 0.999, 1e-8, WD, 1.0, decoupled)
    aerr = 0.0
    for got, ref in ((tr.params, p), (tr.exp_avg, m), (tr.exp_avg_sq, v2)):
        aerr = max(aerr, float((got.double() - ref).abs().max()))
        torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-6)
        assert bool((got[~used] == 0).all()), "padding between arena tensors must stay zero"
    print(f"B={B} M={M} D={D} H={H} Z={Z} beta={beta}: grad err {worst:.2e} adam abs err {aerr:.2e} "
          f"loss {loss} ref {float(f['loss'])}")
    st = tr.read_state()
    assert st["step"] == 3 and st["cursor"] == 0


@pytest.mark.parametrize("B,M,D,H,Z", SHAPES)
def test_eval_and_recon_match_float64_oracle(B, M, D, H, Z):
    """``evaluate`` (the ``backward=False`` path) over two full batches and an
    M-row tail, and ``recon()`` of the first batch."""
    from multidisttorch_amd.models.mlp_vae import reference_forward
    from multidisttorch_amd.ops.philox import reparam_eps

    beta = 0.5
    tr = _trainer(B, D, H, Z, beta)
    X, _ = _data(B, D, seed=5)
    n = 2 * B + M
    total, first = tr.evaluate(X, torch.arange(n, dtype=torch.int32))
    v = {k: t.double() for k, t in tr.named_parameters().items()}
    want = 0.0
    for b in range(3):
        rows = min(B, n - b * B)
        eps = torch.from_numpy(reparam_eps(rows, Z, tr.seed, EVAL_STREAM + tr.rng_stream, b)).double()
        f = reference_forward(v, X[b * B: b * B + rows].double(), eps, beta)
        want += float(f["loss"])
        np.testing.assert_allclose(tr.loss_history(eval=True)[b], float(f["loss"]), rtol=1e-4)
        if b == 0:
            assert first.shape == (B, D)
            # sigmoid is 1/4-Lipschitz; logits of O(1): 1e-5 absolute is ~100 f32 roundings of the logit
            torch.testing.assert_close(first.double(), f["p"], rtol=0, atol=1e-5)
    assert math.isclose(total, want, rel_tol=1e-4), (total, want)
    assert tr.read_state(eval=True)["epoch_count"] == 3
