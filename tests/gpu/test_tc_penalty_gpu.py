"""The total-correlation penalty (``tc_weight``, csrc/kernels/vae_tc.hip) on one
MI355X: the kernels through their binding against the float64 oracle of
models/latent.py, one training step of every trainer form with and without the
penalty, graph replay, and the routing of the 28x28 conv-VAE to the layer path.

Bounds: tests/tc_cases.py (16 times the float32 oracle's own error, floored by
one float32 rounding of the largest value entering the quantity). Every check
prints the achieved error next to its bound.
"""
import numpy as np
import pytest
import torch

from tests import mlp_checker as ck
from tests import tc_cases as tcc

pytestmark = pytest.mark.gpu

BETA = 1.0
TCW = 3.0
HEAD_SCALE = 4.0   # as tests/gpu/test_free_bits_gpu.py: the posteriors of an untrained encoder barely differ
MLP_SCALE = 6.0


def _dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------- kernels through the binding
def _run_kernels(C, mulv, eps, splits, weight=1.0):
    M, Z = eps.shape
    ws = torch.zeros(C.tc_ws_numel(M, Z, splits), device=_dev())
    value = torch.zeros(1, dtype=torch.float64, device=_dev())
    add = torch.full((M, 2 * Z), float("nan"), device=_dev())
    w = torch.tensor([weight], dtype=torch.float32, device=_dev())
    C.tc_penalty(mulv, eps, M, Z, ws, value, weight=w, add_out=add, splits=splits)
    torch.cuda.synchronize()
    return float(value.item()), add.cpu()


_oracles = {}


def _oracle(name, make):
    if name not in _oracles:
        mulv = make()
        eps = tcc.noise(mulv.shape[0], mulv.shape[1] // 2)
        _oracles[name] = (mulv, eps) + tcc.bounds(mulv, eps)
    return _oracles[name]


@pytest.mark.parametrize("name,make", tcc.KERNEL_CASES, ids=[c[0] for c in tcc.KERNEL_CASES])
def test_kernels_match_the_float64_oracle(name, make, native_ext):
    from multidisttorch_amd.ops import native

    C = native.require()
    mulv, eps, v64, g64, bv, bg = _oracle(name, make)
    M, Z = eps.shape
    dm, de = mulv.to(_dev()).contiguous(), eps.to(_dev()).contiguous()
    default = C.tc_default_splits(M, Z)
    worst = 0.0
    for splits in (1, 3, None):
        if splits is not None and splits > (M + 15) // 16:
            with pytest.raises(ValueError):  # outside the domain: the binding raises
                C.tc_ws_numel(M, Z, splits)
            continue
        v, g = _run_kernels(C, dm, de, splits)
        v2, g2 = _run_kernels(C, dm, de, splits)
        assert v == v2 and torch.equal(g, g2), f"{name} splits={splits}: not bitwise repeatable"
        ev, eg = abs(v - v64), float((g.double() - g64).abs().max())
        print(f"tc {name} M={M} Z={Z} splits={splits or default}: value {v:.6g} err {ev:.3g}/{bv:.3g}  "
              f"grad max|g| {float(g64.abs().max()):.4g} err {eg:.3g}/{bg:.3g}")
        assert torch.isfinite(g).all()
        if M == 1:
            assert v == 0.0 and not g.any(), "M = 1: value and gradient are exactly 0"
        assert ev <= bv and eg <= bg, (name, splits, ev, bv, eg, bg)
        worst = max(worst, ev / bv, eg / bg if bg > 0 else 0.0)
    print(f"tc {name}: worst error/bound {worst:.3f}")
    # the weight scales the gradient, not the value
    v, g = _run_kernels(C, dm, de, None, weight=0.0)
    assert abs(v - v64) <= bv and not g.any()


def test_domain_errors(native_ext):
    from multidisttorch_amd.ops import native

    C = native.require()
    for M, Z, s in ((0, 8, None), (4097, 8, None), (16, 0, None), (16, 65, None), (16, 8, 2), (64, 8, 0), (64, 8, 65)):
        with pytest.raises(ValueError):
            C.tc_ws_numel(M, Z, s)


# ---------------------------------------------------------------- one step, every trainer form
_data_cache = {}


def _data(rows, D, seed=7):
    key = (rows, D, seed)
    if key not in _data_cache:
        _data_cache.clear()
        X = torch.rand(rows, D, generator=torch.Generator().manual_seed(seed)).to(_dev())
        _data_cache[key] = (X, torch.arange(rows, device=_dev(), dtype=torch.int32))
    return _data_cache[key]


def _conv(image=28, z=32, B=32, seed=2, graphs=False, nb=4, **kw):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=B, image=image, z=z, device=_dev(), backend="hip", seed=seed, kl_beta=BETA,
                        use_graphs=graphs, graph_steps=3, **kw)
    with torch.no_grad():
        tr.named_parameters()["enc_head.weight"].mul_(HEAD_SCALE)
    tr.refresh_weights()
    X, idx = _data(8 * B, image * image)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, nb)
    return tr


def _conv_once(tr, M):
    """One layer-path step of M rows with the gradients left in the arena (no Adam), then what it stored."""
    assert not tr.f28
    st, C = tr.state, tr.C
    C.step_begin(st.train_state, st.hparams)
    C.gather_rows(tr._data[0], tr._data[1], st.train_state, tr.B, M, tr.xb)
    tr._forward_hip(M, st.train_state, 0)
    tr._backward_hip(M, with_loss=True)
    tr._finalize_grads(M, False)
    torch.cuda.synchronize()
    return dict(mulv=tr.mulv[:M].clone(), eps=tr.eps[:M].clone(), z=tr.z16[:M].clone(), dmulv=tr.dmulv[:M].clone(),
                dmulv16=tr.dmulv16[:M].clone(), hist=tr.loss_history().copy(), state=tr.read_state())


def _mlp(sid, seed=3, graphs=False, **kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    s = ck.SHAPES[sid]
    tr = MlpVaeTrainer(batch_size=s["B"], D=s["D"], H=s["H"], Z=s["Z"], device=_dev(), backend="hip", seed=seed,
                       kl_beta=BETA, use_graphs=graphs, graph_steps=3, **kw)
    with torch.no_grad():
        v = tr.named_parameters()
        v["fc21.weight"].mul_(MLP_SCALE)
        v["fc22.weight"].mul_(MLP_SCALE)
    X, idx = _data(8 * s["B"], s["D"])
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 4)
    return tr


def _mlp_once(tr, M):
    e = tr.engine
    e.forward(tr._data[0], tr._data[1], M, True, False, 5, False)
    tr._tc_step(M)
    e.backward(tr._data[0], tr._data[1], M, 0, False)
    torch.cuda.synchronize()
    s = {n: e.act(n, M).clone() for n in ("mulv", "eps", "z", "dmulv", "dh1")}
    s.update(hist=tr.loss_history().copy(), state=tr.read_state())
    return s


def _check_step(s0, s1, Z, label):
    for k in ("mulv", "eps", "z"):
        assert torch.equal(s0[k], s1[k]), k
    np.testing.assert_array_equal(s0["hist"], s1["hist"])  # the loss ring keeps meaning BCE + kl_t * KL
    assert s0["state"]["epoch_loss"] == s1["state"]["epoch_loss"]
    v64, g64, bv, bg = tcc.bounds(s0["mulv"].cpu(), s0["eps"].cpu())
    d0, d1 = s0["dmulv"].double().cpu(), s1["dmulv"].double().cpu()
    tol = TCW * bg + 2 * tcc.U32 * torch.maximum(d0.abs(), d1.abs())
    err = ((d1 - d0) - TCW * g64).abs()
    miss = (TCW * g64).abs()  # the same check on the step without the penalty
    ev = abs(s1["state"]["epoch_tc"] - v64)
    print(f"tc step {label}: max|g| {float(g64.abs().max()):.4g}  dmulv err/tol {float((err / tol).max()):.3g}  "
          f"(max err {float(err.max()):.3g}, gradient bound {bg:.3g})  without the penalty {float((miss / tol).max()):.3g}  "
          f"epoch_tc {s1['state']['epoch_tc']:.6g} err {ev:.3g}/{bv:.3g}")
    assert bool((err <= tol).all()), float((err / tol).max())
    assert not bool((miss <= tol).all()), "the step without the penalty passes the same check: no power"
    assert ev <= bv, (s1["state"]["epoch_tc"], v64, bv)
    assert s0["state"]["epoch_tc"] == 0.0 and s0["state"]["tc_weight"] == 0.0
    assert s1["state"]["tc_weight"] == TCW
    return g64


@pytest.mark.parametrize("sid,M", [("default", 128), ("default", 37), ("ragged", 37)])
def test_mlp_step_adds_the_penalty_gradient(sid, M, native_ext):
    Z = ck.SHAPES[sid]["Z"]
    s0 = _mlp_once(_mlp(sid), M)
    s1 = _mlp_once(_mlp(sid, tc_weight=TCW), M)
    _check_step(s0, s1, Z, f"mlp {sid} M={M}")
    assert not torch.equal(s0["dh1"], s1["dh1"])  # added before the dh1 product


@pytest.mark.parametrize("image,z,B,M", [(28, 32, 32, 32), (28, 32, 32, 13), (28, 16, 32, 32), (28, 16, 32, 13),
                                         (128, 64, 16, 16), (128, 64, 16, 13)])
def test_conv_layer_path_adds_the_penalty_gradient(image, z, B, M, native_ext, monkeypatch):
    """28x28 at Z = 32 and Z = 16 (the row-form and the strided split-K combine) and 128x128."""
    monkeypatch.setenv("MDT_CONV_F28", "0")  # the step without the penalty on the layer path too
    s0 = _conv_once(_conv(image, z, B), M)
    s1 = _conv_once(_conv(image, z, B, tc_weight=TCW), M)
    _check_step(s0, s1, z, f"conv{image} Z={z} M={M}")
    assert torch.equal(s1["dmulv16"].float(), s1["dmulv"].to(torch.bfloat16).float())  # the bf16 copy follows


# ---------------------------------------------------------------- graphs
def _make(kind, **kw):
    if kind == "mlp":
        return _mlp("default", 2, **kw)
    if kind == "c128":
        return _conv(128, 64, 8, **kw)
    return _conv(**kw)


def _state_of(tr, steps):
    torch.cuda.synchronize()
    st = tr.read_state()
    assert st["step"] == steps
    h = tr.loss_history()[:steps].copy()
    assert np.isfinite(h).all() and np.isfinite(st["epoch_tc"])
    return h, tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), st


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4], (a[4], b[4])


@pytest.mark.parametrize("kind,tail", [("conv28", 13), ("c128", 5), ("mlp", 13)])
def test_eager_equals_graph_replay(kind, tail, native_ext):
    res = []
    for graphs in (False, True):
        tr = _make(kind, graphs=graphs, tc_weight=TCW)
        tr.train_steps(6)            # 2 * graph_steps
        tr.train_steps(1, tail)
        res.append(_state_of(tr, 7))
        assert res[-1][4]["tc_weight"] == TCW and res[-1][4]["epoch_tc"] != 0.0
    _same(res[0], res[1])
    tr = _make(kind, graphs=True)    # and the penalty is in force: a trainer without it ends elsewhere
    tr.train_steps(6)
    tr.train_steps(1, tail)
    assert not torch.equal(_state_of(tr, 7)[1], res[0][1])


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_eval_passes_leave_the_training_untouched(kind, native_ext, monkeypatch):
    monkeypatch.setenv("MDT_CONV_F28", "0")  # the trainer without the penalty evaluates on the layer path too
    a, b = _make(kind, graphs=True, tc_weight=TCW), _make(kind, graphs=True, tc_weight=TCW)
    X, idx = a._data[0], a._data[1]
    ev = idx[: a.B + 5]
    a.train_steps(3)
    loss, _ = a.evaluate(X, ev, want_first_recon=False)
    # the test loss is the true ELBO: a trainer without the penalty scores the same weights the same
    # (both in their first evaluation: the eval noise follows the eval state's step)
    c = _make(kind, graphs=True)
    c.load_state_dict(a.state_dict())
    assert c.evaluate(X, ev, want_first_recon=False)[0] == loss
    a.evaluate_iw(X, ev, 4)
    rep = a.evaluate_latent(X, ev)
    assert a.read_state(eval=True)["tc_weight"] == 0.0 and loss == loss and np.isfinite(rep["tc"])
    a.train_steps(3)
    b.train_steps(6)
    _same(_state_of(a, 6), _state_of(b, 6))


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_graph_picks_up_a_new_weight(kind, native_ext):
    g, e = _make(kind, graphs=True, tc_weight=TCW), _make(kind, tc_weight=TCW)
    for tr in (g, e):
        tr.train_steps(3)
        tr.set_hparams(tc_weight=2 * TCW)
        tr.train_steps(3)
        assert tr.read_state()["tc_weight"] == 2 * TCW
        tr.set_hparams(tc_weight=0.0)
        tr.train_steps(3)
        assert tr.read_state()["tc_weight"] == 0.0
    _same(_state_of(g, 9), _state_of(e, 9))
    k = _make(kind, graphs=True, tc_weight=TCW)  # each change mattered
    k.train_steps(9)
    assert not torch.equal(_state_of(k, 9)[1], g.params)
    with pytest.raises(ValueError):
        _make(kind).set_hparams(tc_weight=1.0)   # built without the penalty's launches


# ---------------------------------------------------------------- routing
def test_the_penalty_routes_28x28_to_the_layer_path(native_ext):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    kw = dict(batch_size=16, image=28, z=32, device=_dev(), backend="hip")
    assert ConvVaeTrainer(**kw).f28 is True
    assert ConvVaeTrainer(tc_weight=1.0, **kw).f28 is False
