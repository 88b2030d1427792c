"""Latent report on the HIP backends (csrc/kernels/vae_latent.hip;
``evaluate_latent`` of both trainers). Inputs and bounds: tests/latent_cases.py.

Bounds, none of them taken from the code under test:
  * every scalar, per-dimension vector and per-row lq_joint / lq_marg / lq_cond
    / lp against the float64 oracle (models/latent.py) fed with the device's
    eps: 16 x the error of the float32 torch oracle against the float64 one on
    the same input, per quantity, measured on the CPU inside the test (and
    never taken below one float32 rounding of the values that enter the
    quantity, see latent_cases.bounds). On the CPU the float32 oracle's error
    was at most 3.8e-4 on the per-row values (sharp, Z = 64, values to 260)
    and 2.2e-5 on the scalars, so the bounds there are 6.1e-3 and 2.1e-4 to
    3.5e-4. Achieved on an MI355X: 3.9e-4 per row and 1.5e-5 (tc) on the same
    input; over all inputs and trainer passes the largest error / bound ratio
    was 0.20 (lq_marg, mixed, Z = 64), for mi 0.013;
  * device eps against host ``reparam_eps``: rtol = atol = 1e-5, the project's
    Philox bound (test_philox_host_matches_device);
  * 1 split against 3 splits: the same bound; each bitwise repeatable;
  * mulv of the pass against the importance-weighted pass's: bitwise;
  * graphed against eager, and 3 steps + passes + 3 steps against 6 steps: bitwise.
Each check prints the achieved error next to its bound.
"""
import math

import numpy as np
import pytest
import torch

from tests import latent_cases as lc

pytestmark = pytest.mark.gpu

SEED = 7
MIXED = [(85, 20), (117, 32), (53, 64)]
_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _images(n, size=28):
    from multidisttorch_amd.data.datasets import synthetic_images

    key = (n, size)
    if key not in _cache:
        _cache[key] = synthetic_images(n, size=size, seed=5, device=_dev())
    return _cache[key]


def _mlp(B=32, graphs=False, **kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    return MlpVaeTrainer(batch_size=B, device=_dev(), backend="hip", seed=SEED, use_graphs=graphs, graph_steps=3, **kw)


def _conv(B=32, image=28, graphs=False, **kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    return ConvVaeTrainer(batch_size=B, image=image, z=32 if image == 28 else 64, device=_dev(), backend="hip",
                          seed=SEED, use_graphs=graphs, graph_steps=3, **kw)


def _train(tr, X, steps):
    n = X.shape[0] // tr.B * tr.B
    tr.bind_train_data(X, torch.arange(n, dtype=torch.int32, device=X.device))
    tr.set_cursor(0, n // tr.B)
    tr.train_steps(steps)
    torch.cuda.synchronize()


def _arange(n):
    return torch.arange(n, dtype=torch.int32, device=_dev())


def _report(mulv, splits=None, au_threshold=0.01):
    """The kernels alone on synthetic rows: the dict ``evaluate_latent`` returns
    (with rows), plus ``eps``."""
    C = _C()
    n, Z = mulv.shape[0], mulv.shape[1] // 2
    rows = mulv.to(_dev()).contiguous()
    st = C.latent_state_new(0)
    C.latent_state_begin(st, 1)
    hp = C.latent_hparams(SEED, 0)
    nf, nd = C.latent_ws_numel(n, Z, splits)
    ws = [torch.zeros(nf, dtype=torch.float32, device=_dev()), torch.zeros(nd, dtype=torch.float64, device=_dev())]
    C.latent_report(rows, n, Z, st, hp, ws, splits)
    torch.cuda.synchronize()
    r = C.latent_state_read(st)
    view = lambda name: C.latent_ws_view(ws[0], n, Z, splits, name).clone().cpu()
    out = dict(rows=n, kl=r[0], mi=r[1], tc=r[2], dwkl=r[3], sampled_kl=r[4], au_threshold=au_threshold)
    for k in lc.VECTORS + lc.ROWS + ("eps", "z"):
        out[k] = view(k)
    out["active_units"] = int((out["mu_var"] > au_threshold).sum())
    return out


def _check_eps(eps, n, Z):
    from multidisttorch_amd.ops.philox import reparam_eps

    np.testing.assert_allclose(eps.numpy(), reparam_eps(n, Z, SEED, 3 << 28, 0), rtol=1e-5, atol=1e-5)


def _kernel_cases():
    off = lambda m: torch.cat([m[:, : m.shape[1] // 2] + 100.0, m[:, m.shape[1] // 2:]], 1)
    cases = [("overlap", lc.overlap)]
    for n, Z in MIXED:
        cases.append((f"mixed{n}x{Z}", lambda n=n, Z=Z: lc.mixed(n, Z)))
        cases.append((f"sharp{n}x{Z}", lambda n=n, Z=Z: lc.sharp(n, Z)))
        cases.append((f"offset{n}x{Z}", lambda n=n, Z=Z: off(lc.mixed(n, Z))))
    return cases


@pytest.mark.parametrize("name,make", _kernel_cases(), ids=[c[0] for c in _kernel_cases()])
def test_kernels_match_float64_oracle(name, make, native_ext):
    mulv = make()
    n, Z = mulv.shape[0], mulv.shape[1] // 2
    got = _report(mulv)
    _check_eps(got["eps"], n, Z)
    o64, bound = lc.bounds(mulv, got["eps"])
    lc.check(got, o64, bound, name)
    if name == "overlap":
        assert o64["mi"] < 0.8 * math.log(n)  # a wrong MI cannot hide behind the log n ceiling
    if name.startswith("mixed") or name.startswith("offset"):
        assert got["active_units"] == Z // 4
    if name == "sharp53x64":
        assert lc.max_joint(mulv, got["eps"]) > 88.7  # exp() of it overflows float32


def test_one_row(native_ext):
    mulv = lc.mixed(1, 20)
    got = _report(mulv)
    o64, bound = lc.bounds(mulv, got["eps"])
    lc.check(got, o64, bound, "n=1")
    assert got["mi"] == 0.0 and got["tc"] == 0.0 and got["dwkl"] == got["sampled_kl"]
    assert got["active_units"] == 0


def test_splits_agree_and_repeat_bitwise(native_ext):
    """n = 257 is no multiple of the 64-row i tile or the 16-row j tile and
    spans 17 j tiles; forced to 1 and to 3 j-splits."""
    mulv = lc.mixed(257, 20)
    runs = {s: [_report(mulv, splits=s) for _ in range(2)] for s in (1, 3, None)}
    o64, bound = lc.bounds(mulv, runs[1][0]["eps"])
    for s, (a, b) in runs.items():
        lc.check(a, o64, bound, f"n=257 splits={s}")
        for k in lc.SCALARS:
            assert a[k] == b[k], (s, k)
        for k in lc.VECTORS + lc.ROWS:
            assert torch.equal(a[k], b[k]), (s, k)
    a, b = runs[1][0], runs[3][0]
    for k in lc.SCALARS:
        assert abs(a[k] - b[k]) <= bound[k], k
    for k in ("lq_joint", "lq_marg"):
        assert float((a[k] - b[k]).abs().max()) <= bound[k], k
    assert torch.equal(a["lq_cond"], b["lq_cond"]) and torch.equal(a["kl_per_dim"], b["kl_per_dim"])
    assert _C().latent_default_splits(257) == 17 and _C().latent_default_splits(10000) == 13


def test_out_of_domain_arguments_raise(native_ext):
    C = _C()
    for n, Z, splits in ((10, 65, None), (10, 0, None), (0, 4, None), (2 ** 32 // 64 + 1, 64, None), (40, 4, 0),
                         (40, 4, 4), (2000, 4, 65)):
        with pytest.raises((ValueError, RuntimeError)):
            C.latent_ws_numel(n, Z, splits)
    mulv = lc.overlap().to(_dev())
    st, hp = C.latent_state_new(0), C.latent_hparams(SEED, 0)
    nf, nd = C.latent_ws_numel(40, 4)
    ws = [torch.zeros(nf, device=_dev()), torch.zeros(nd, dtype=torch.float64, device=_dev())]
    with pytest.raises((ValueError, RuntimeError)):
        C.latent_report(mulv, 40, 4, st, hp, ws, 4)          # 40 rows are 3 j tiles
    with pytest.raises((ValueError, RuntimeError)):
        C.latent_report(mulv, 41, 4, st, hp, ws)             # more rows than the buffer holds
    with pytest.raises((ValueError, RuntimeError)):
        C.latent_report(mulv, 40, 4, st, hp, [ws[0][:100], ws[1]])
    with pytest.raises(ValueError):
        _mlp().evaluate_latent(_images(64), _arange(0))


def _pass_checks(tr, X, n, label):
    idx = _arange(n)
    tr.evaluate_iw(X, idx, 1)
    torch.cuda.synchronize()
    M = n - (-(-n // tr.B) - 1) * tr.B
    iw_mulv = tr.iw_buffers(1, M)["mulv"].clone()
    r = tr.evaluate_latent(X, idx, return_rows=True)
    torch.cuda.synchronize()
    buf = tr.latent_buffers()
    assert buf["mulv"].shape == (n, 2 * tr.Z)
    assert torch.equal(buf["mulv"][n - M:], iw_mulv), "the pass's rows are not the importance-weighted pass's"
    eps = buf["eps"].cpu()
    _check_eps(eps, n, tr.Z)
    o64, bound = lc.bounds(buf["mulv"].cpu(), eps)
    lc.check(r, o64, bound, label)
    return r


@pytest.mark.parametrize("n", [85, 117])
def test_mlp_pass_matches_float64_oracle(n, native_ext):
    X = _images(256)
    tr = _mlp(32)
    _train(tr, X, 30)
    r = _pass_checks(tr, X, n, f"mlp n={n}")
    assert r["rows"] == n and r["kl"] > 0 and 0 <= r["mi"] <= math.log(n) + 1e-3


@pytest.mark.parametrize("image,B,n", [(28, 32, 53), (128, 16, 21)])
def test_conv_pass_matches_float64_oracle(image, B, n, native_ext):
    X = _images(64, image)
    tr = _conv(B, image)
    _train(tr, X, 4)
    _pass_checks(tr, X, n, f"conv{image} n={n}")


@pytest.mark.parametrize("kind,image,B,n", [("mlp", 28, 32, 85), ("conv", 28, 32, 53), ("conv", 128, 16, 21)])
def test_degenerate_identity(kind, image, B, n, native_ext):
    """A zero encoder head: mu = lv = 0 for every row, so q(z|x) = p(z): no KL,
    no active unit, no information, no correlation, and the sampled KL is all
    dimension-wise (n equal terms under every log-sum-exp: exactly)."""
    X = _images(256 if kind == "mlp" else 64, image)
    tr = _mlp(B) if kind == "mlp" else _conv(B, image)
    v = tr.named_parameters()
    for name in (("fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias") if kind == "mlp" else
                 ("enc_head.weight", "enc_head.bias")):
        v[name].zero_()
    tr.refresh_weights()
    r = tr.evaluate_latent(X, _arange(n))
    torch.cuda.synchronize()
    print({k: r[k] for k in lc.SCALARS}, "active", r["active_units"])
    assert float(tr.latent_buffers()["mulv"].abs().max()) == 0.0
    assert r["kl"] == 0.0 and r["active_units"] == 0 and float(r["mu_var"].abs().max()) == 0.0
    assert r["mi"] == 0.0 and r["tc"] == 0.0 and r["dwkl"] == r["sampled_kl"]
    assert float((r["post_var"] - 1.0).abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_graphed_pass_is_bitwise_eager_and_repeatable(kind, native_ext):
    X = _images(256)
    n = 117  # batches 32, 32, 32 (batch 0 eager, one graph of two) and a tail of 21 (a graph of its own)
    out = {}
    for graphs in (False, True):
        tr = _mlp(32, graphs) if kind == "mlp" else _conv(32, 28, graphs)
        _train(tr, X, 3)
        res = []
        for _ in range(2):
            r = tr.evaluate_latent(X, _arange(n), return_rows=True)
            torch.cuda.synchronize()
            res.append((tuple(r[k] for k in lc.SCALARS), [r[k].cpu() for k in lc.VECTORS + lc.ROWS],
                        tr.latent_buffers()["mulv"].cpu()))
        out[graphs] = res
        if graphs:
            assert sorted(tr._lat_graphs) == [(1, 21), (2, 32)], "the graphed path did not run"
    a0, a1 = out[False]
    for b in (a1, *out[True]):
        assert a0[0] == b[0], (a0[0], b[0])
        assert all(torch.equal(x, y) for x, y in zip(a0[1], b[1])) and torch.equal(a0[2], b[2])
    assert all(math.isfinite(x) for x in a0[0])


@pytest.mark.parametrize("kind", ["mlp", "conv28"])
def test_training_continues_bitwise_after_the_passes(kind, native_ext):
    """3 steps + evaluate + evaluate_iw + evaluate_latent + 3 steps == 6 steps,
    bitwise, and the latent pass leaves the train and eval states, their loss
    rings and the iw pass alone."""
    X = _images(256)
    make = (lambda: _mlp(32, True)) if kind == "mlp" else (lambda: _conv(32, 28, True))
    a, b = make(), make()
    _train(a, X, 6)
    _train(b, X, 3)
    b.evaluate(X, _arange(53), want_first_recon=False)
    iw0 = b.evaluate_iw(X, _arange(53), 3, chunk_samples=2)
    torch.cuda.synchronize()
    before = (b.read_state(), b.read_state(eval=True), b.loss_history().copy(), b.loss_history(eval=True).copy())
    b.evaluate_latent(X, _arange(53))
    torch.cuda.synchronize()
    after = (b.read_state(), b.read_state(eval=True), b.loss_history(), b.loss_history(eval=True))
    assert before[0] == after[0] and before[1] == after[1]
    np.testing.assert_array_equal(before[2], after[2])
    np.testing.assert_array_equal(before[3], after[3])
    assert b.evaluate_iw(X, _arange(53), 3, chunk_samples=2) == iw0
    b.train_steps(3)
    torch.cuda.synchronize()
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.read_state() == b.read_state()
