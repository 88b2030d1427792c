"""The MLP-VAE kernels (csrc/kernels/vae_mlp.hip, tile_gemm.h, vae_iw.hip,
adam.hip) over the shape domain the engine accepts, not only D=784, H=400, Z=20.

* ``test_stages_match_float64``: every stored stage of forward + backward against
  float64 recomputed from the device's own inputs of that stage, with the derived
  bounds of tests/mlp_checker.py (the table of shapes and which path each one
  reaches is there).
* ``test_*_exact``: the long reductions (F1/B1 at D = 1156 and 16384, the weight
  gradients at M up to 4096) with operands whose every partial sum is an f32
  number: the result equals float64 bit for bit in any summation order, so a
  dropped k-chunk or row pair cannot hide in the bound.
* the whole step at the new shapes: fused Adam, graph replay, eval + decode, the
  importance-weighted pass.
* unsupported shapes are refused at construction, by name.
"""

import math

import numpy as np
import pytest
import torch

from tests import mlp_checker as ck

pytestmark = pytest.mark.gpu

SEED = 3
EVAL_STREAM = 1 << 30
IW_STREAM = 1 << 29
# KL weights other than 1 (exact in f32, so the float64 reference uses the kernels' value)
BETA = {"ragged": 0.5, "wide": 4.0, "img128": 0.5, "brounds": 4.0, "bmax": 0.5}
STEP_IDS = ("tiny", "ragged", "wide", "img128", "brounds")


def _dev():
    return torch.device("cuda", 0)


def _trainer(sid, graphs=False, **kw):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    s = ck.SHAPES[sid]
    kw.setdefault("kl_beta", BETA.get(sid, 1.0))
    return MlpVaeTrainer(batch_size=s["B"], D=s["D"], H=s["H"], Z=s["Z"], device=_dev(), backend="hip", seed=SEED,
                         use_graphs=graphs, graph_steps=2, **kw)


_cache = {}


def _data(sid, nb=2):
    """(X[nb*B + 7, D], idx[nb*B]) on the device: nb batches of a shuffled index list."""
    key = (sid, nb)
    if key not in _cache:
        _cache.clear()  # one shape's data at a time (the D = 16384 sets are tens of MB)
        s = ck.SHAPES[sid]
        g = torch.Generator().manual_seed(SEED)
        n = nb * s["B"] + 7
        X = torch.rand(n, s["D"], generator=g)
        idx = torch.randperm(n, generator=g)[: nb * s["B"]].to(torch.int32)
        _cache[key] = (X.to(_dev()), idx.to(_dev()))
    return _cache[key]


def _report(tag, ratios):
    print(tag, "worst error/bound per stage:", " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _used(tr):
    used = torch.zeros(tr.numel, dtype=torch.bool, device=tr.params.device)
    for _, o, s in tr.layout:
        used[o: o + math.prod(s)] = True
    return used


# ------------------------------------------------ 2. stage-wise shape sweep ----
@pytest.mark.parametrize("sid,M", ck.cases())
def test_stages_match_float64(sid, M, native_ext):
    from multidisttorch_amd.ops.philox import reparam_eps

    s = ck.SHAPES[sid]
    B, Z = s["B"], s["Z"]
    beta = BETA.get(sid, 1.0)
    tr = _trainer(sid)
    X, idx = _data(sid)
    tr.bind_train_data(X, idx)
    tr.set_cursor(1, 2)  # the second batch: the kernels index idx at cursor * B
    e = tr.engine
    e.forward(X, idx, M, True, False, 5, True)
    fwd_only = bool(s.get("forward_only"))
    if fwd_only:
        e.loss_finalize(False)
    else:
        e.backward(X, idx, M, 0, False)
    torch.cuda.synchronize()
    x = X[idx[B: B + M].long()].cpu()
    v = {k: t.cpu() for k, t in tr.named_parameters().items()}
    names = ["h1", "mulv", "eps", "z", "h3", "recon", "dlog"] + ([] if fwd_only else ["dh3", "dmulv", "dh1"])
    dev = {n: e.act(n, M).cpu() for n in names}
    # the batch rows F1 copied for F3 / B3, and nothing stored past row M
    assert torch.equal(e.act("xb", M).cpu(), x)
    if M < B:
        for n in names:
            assert not bool(e.act(n, B)[M:].any()), f"{n}: rows >= M written"
    loss = float(tr.loss_history()[0])
    r = ck.check_forward(dev, v, x, beta, reparam_eps(M, Z, SEED, 5, 0), loss)
    if not fwd_only:
        g = {k: t.cpu() for k, t in tr.named_grads().items()}
        r.update(ck.check_backward(dev, g, v, x, beta))
        assert not bool(tr.grads[~_used(tr)].any()), "padding of the gradient arena written"
    _report(f"{sid} M={M}", r)
    st = tr.read_state()
    assert st["step"] == 1 and st["cursor"] == 0 and st["kl_beta"] == beta


# ------------------------------- 3. exact arithmetic on the long reductions ----
def _plant(t, value):
    t.copy_(value.to(t.device))


@pytest.mark.parametrize("sid,M", ck.cases(ids=tuple(ck.EXACT_D.values())))
def test_f1_exact(sid, M, native_ext):
    """h1 = relu(X W1^T + b1) over K = D and [mu|lv] = h1 W2^T + b2 over the H/16 slabs,
    on integer operands (W2 in units of 2^-20, b2 of 2^-3, so mu and lv stay within +-1)."""
    s = ck.SHAPES[sid]
    B, D, H, Z = s["B"], s["D"], s["H"], s["Z"]
    assert D in ck.EXACT_D
    g = torch.Generator().manual_seed(7)
    tr = _trainer(sid)
    X = ck.randint(g, (2 * B, D), 0, 1)
    idx = torch.randperm(2 * B, generator=g)[:B].to(torch.int32)
    W1, b1 = ck.randint(g, (H, D), -1, 1), ck.randint(g, (H,), -3, 3)
    W2, b2 = ck.randint(g, (2 * Z, H), -1, 1) * 2.0 ** -20, ck.randint(g, (2 * Z,), -4, 4) * 2.0 ** -3
    v = tr.named_parameters()
    _plant(v["fc1.weight"], W1), _plant(v["fc1.bias"], b1)
    _plant(v["fc21.weight"], W2[:Z]), _plant(v["fc22.weight"], W2[Z:])
    _plant(v["fc21.bias"], b2[:Z]), _plant(v["fc22.bias"], b2[Z:])
    x = X[idx[:M].long()]
    assert ck.exact_ok(x, W1.t(), b1)
    h1 = torch.relu(ck.gemm_ref(x, W1.t(), b1)[0])
    assert ck.exact_ok(h1, W2.t(), b2, lsb=2.0 ** -20)
    mulv = ck.gemm_ref(h1, W2.t(), b2)[0]
    assert float(mulv.abs().max()) <= 1.0
    Xd, idxd = X.to(_dev()), idx.to(_dev())
    tr.bind_train_data(Xd, idxd)
    tr.set_cursor(0, 1)
    tr.engine.forward(Xd, idxd, M, True, False, 0, False)
    torch.cuda.synchronize()
    got_h1, got_mulv = tr.engine.act("h1", M).cpu().double(), tr.engine.act("mulv", M).cpu().double()
    print(f"{sid} M={M}: h1 max {float(h1.max()):.0f}, mismatches h1 {int((got_h1 != h1).sum())} "
          f"mulv {int((got_mulv != mulv).sum())}")
    assert torch.equal(got_h1, h1)
    assert torch.equal(got_mulv, mulv)
    assert math.isfinite(float(tr.engine.act("h3", M).sum()))


@pytest.mark.parametrize("sid,M", ck.cases(ids=tuple(ck.EXACT_D.values())))
def test_b1_exact(sid, M, native_ext):
    """dh3 = (dlog W4) . [h3 > 0] over K = D on planted {-1, 0, 1} operands."""
    s = ck.SHAPES[sid]
    D, H = s["D"], s["H"]
    g = torch.Generator().manual_seed(8)
    tr = _trainer(sid)
    X, idx = _data(sid)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 2)
    e = tr.engine
    e.forward(X, idx, M, True, False, 0, False)
    dlog, h3, W4 = ck.randint(g, (M, D), -1, 1), ck.randint(g, (M, H), 0, 1), ck.randint(g, (D, H), -1, 1)
    _plant(e.act("dlog", M), dlog), _plant(e.act("h3", M), h3), _plant(tr.named_parameters()["fc4.weight"], W4)
    assert ck.exact_ok(dlog, W4)
    ref = ck.gemm_ref(dlog, W4)[0] * (h3 > 0)
    e.backward(X, idx, M, 1, False)
    torch.cuda.synchronize()
    got = e.act("dh3", M).cpu().double()
    print(f"{sid} M={M}: dh3 max {float(ref.abs().max()):.0f}, mismatches {int((got != ref).sum())}")
    assert torch.equal(got, ref)


@pytest.mark.parametrize("sid,M", ck.cases(ids=("brounds", "bmax")))
def test_weight_gradients_exact(sid, M, native_ext):
    """All eight gradient GEMMs over K = M on planted small integers. The inputs of
    a part are planted immediately before that part alone is launched (part 2's
    row blocks rewrite dmulv and dh1)."""
    s = ck.SHAPES[sid]
    D, H, Z = s["D"], s["H"], s["Z"]
    assert M in ck.EXACT_M
    g = torch.Generator().manual_seed(9)
    tr = _trainer(sid)
    X, idx = _data(sid)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 2)
    e = tr.engine
    e.forward(X, idx, M, True, False, 0, False)
    ones = torch.ones(M, 1)

    def run(part, dys, acts, outs):
        planted = {}
        for n, (lo, hi) in {**dys, **acts}.items():
            planted[n] = ck.randint(g, tuple(e.act(n, M).shape), lo, hi)
            _plant(e.act(n, M), planted[n])
        e.backward(X, idx, M, part, False)
        torch.cuda.synchronize()
        gr = {k: t.cpu().double() for k, t in tr.named_grads().items()}
        for (dy, a), (wn, bn) in zip(zip(dys, acts), outs):
            A, Bm = planted[dy].t().contiguous(), planted[a]
            assert ck.exact_ok(A, Bm) and ck.exact_ok(A, ones)
            gw, gb = torch.cat([gr[n] for n in wn], 0), torch.cat([gr[n] for n in bn], 0)
            rw, rb = ck.gemm_ref(A, Bm)[0], ck.gemm_ref(A, ones)[0][:, 0]
            print(f"{sid} M={M} {wn[0]}: max {float(rw.abs().max()):.0f}, mismatches "
                  f"{int((gw != rw).sum())} bias {int((gb != rb).sum())}")
            assert torch.equal(gw, rw), wn
            assert torch.equal(gb, rb), bn

    run(2, {"dlog": (-1, 1), "dh3": (-1, 1)}, {"h3": (0, 3), "z": (0, 3)},
        [(["fc4.weight"], ["fc4.bias"]), (["fc3.weight"], ["fc3.bias"])])
    run(3, {"dmulv": (-1, 1), "dh1": (-1, 1)}, {"h1": (0, 3), "xb": (0, 3)},
        [(["fc21.weight", "fc22.weight"], ["fc21.bias", "fc22.bias"]), (["fc1.weight"], ["fc1.bias"])])


# ------------------------------------------ 4. the whole step at new shapes ----
ADAM = {"tiny": dict(weight_decay=0.01, decoupled_wd=False, grad_scale=0.5),  # coupled decay, scaled gradients
        "ragged": dict(weight_decay=0.01, decoupled_wd=True)}                  # AdamW


@pytest.mark.parametrize("sid", STEP_IDS)
def test_fused_adam_matches_unfused_gradients_and_float64_adam(sid, native_ext):
    from multidisttorch_amd.models.mlp_vae import reference_adam_

    s = ck.SHAPES[sid]
    M = s["Ms"][-1]
    kw = dict(ADAM.get(sid, {}))
    gs = kw.pop("grad_scale", 1.0)
    tr = _trainer(sid, lr=2e-3, **kw)
    tr.set_hparams(grad_scale=gs)
    X, idx = _data(sid)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 2)
    used = _used(tr)
    # optimizer state as two earlier steps could have left it (v >= m^2), on the tensors only
    g = torch.Generator().manual_seed(11)
    m0 = (torch.rand(tr.numel, generator=g) - 0.5) * 1e-2
    v0 = m0 ** 2 + torch.rand(tr.numel, generator=g) * 1e-4
    tr.exp_avg.copy_(m0.to(_dev()) * used)
    tr.exp_avg_sq.copy_(v0.to(_dev()) * used)
    tr.set_step(2)
    e = tr.engine
    p0, m0, v0, st0 = tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), e.state.train_state.clone()
    e.forward(X, idx, M, True, False, 0, False)
    e.backward(X, idx, M, 0, False)
    torch.cuda.synchronize()
    g_unfused = tr.grads.clone()
    assert torch.equal(tr.params, p0) and torch.equal(tr.exp_avg, m0)
    e.state.train_state.copy_(st0)
    tr.grads.zero_()
    e.forward(X, idx, M, True, False, 0, False)
    e.backward(X, idx, M, 0, True)
    torch.cuda.synchronize()
    assert tr.step_count == 3
    assert torch.equal(tr.grads, g_unfused), "fused and unfused gradient arenas differ"
    p, m, v = p0.cpu().double(), m0.cpu().double(), v0.cpu().double()
    reference_adam_(p, g_unfused.cpu().double(), m, v, 3, 2e-3, 0.9, 0.999, 1e-8, kw.get("weight_decay", 0.0), gs,
                    kw.get("decoupled_wd", False))
    for name, got, ref in (("params", tr.params, p), ("exp_avg", tr.exp_avg, m), ("exp_avg_sq", tr.exp_avg_sq, v)):
        d = (got.cpu().double() - ref).abs()
        print(f"{sid} M={M} {name}: max abs err {float(d.max()):.3g}, max err/(1e-6 + 1e-5 |ref|) "
              f"{float((d / (1e-6 + 1e-5 * ref.abs())).max()):.3g}")
        torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-5, atol=1e-6)
    for t in (tr.params, tr.grads, tr.exp_avg, tr.exp_avg_sq):
        assert not bool(t[~used].any()), "padding between arena tensors must stay zero"


@pytest.mark.parametrize("sid", STEP_IDS)
def test_graph_replay_equals_eager(sid, native_ext):
    s = ck.SHAPES[sid]
    X, _ = _data(sid, 3)
    n = 3 * s["B"]
    idx = torch.arange(n, dtype=torch.int32, device=_dev())
    outs = []
    for graphs in (False, True):
        tr = _trainer(sid, graphs=graphs)
        tr.bind_train_data(X, idx)
        tr.set_cursor(0, 3)
        tr.train_steps(5)
        torch.cuda.synchronize()
        st = tr.read_state()
        assert st["step"] == 5 and st["cursor"] == 2
        outs.append((tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.loss_history()[:5].copy()))
        del tr
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    assert np.isfinite(outs[0][3]).all()
    np.testing.assert_array_equal(outs[0][3], outs[1][3])


@pytest.mark.parametrize("sid", STEP_IDS)
def test_eval_with_tail_batch_and_decode(sid, native_ext):
    """``evaluate`` over 2 B + tail rows against the float64 loss sum (relative 2e-5,
    the project's eval bound; 1e-4, the stage-wise loss bound, at D = 16384), which pins
    the tail batch's partial-slot counts at the new tile counts; ``decode`` stage-wise."""
    from multidisttorch_amd.models.mlp_vae import reference_forward
    from multidisttorch_amd.ops.philox import reparam_eps

    s = ck.SHAPES[sid]
    B, Z = s["B"], s["Z"]
    tail = s["Ms"][-1]
    n = 2 * B + tail
    rel = ck.LOSS_REL if sid == "img128" else 2e-5
    X, _ = _data(sid, 3)
    tr = _trainer(sid)
    total, first = tr.evaluate(X, torch.arange(n, dtype=torch.int32, device=_dev()))
    assert first.shape == (B, s["D"])
    v = {k: t.cpu().double() for k, t in tr.named_parameters().items()}
    want = []
    for b in range(3):
        rows = min(B, n - b * B)
        eps = torch.from_numpy(reparam_eps(rows, Z, SEED, EVAL_STREAM, b)).double()
        want.append(float(reference_forward(v, X[b * B: b * B + rows].cpu().double(), eps, BETA.get(sid, 1.0))["loss"]))
    got = tr.loss_history(eval=True)[:3]
    print(f"{sid}: eval loss rel err per batch {[abs(float(a) - w) / w for a, w in zip(got, want)]}, "
          f"sum {abs(total - sum(want)) / sum(want):.3g} (bound {rel})")
    np.testing.assert_allclose(got, want, rtol=rel)
    assert math.isclose(total, sum(want), rel_tol=rel), (total, sum(want))
    assert tr.read_state(eval=True)["epoch_count"] == 3
    # decode: h3 = relu(z W3^T + b3), then sigmoid(h3 W4^T + b4) from the device's h3
    z = torch.randn(tail, Z, generator=torch.Generator().manual_seed(4))
    out = tr.decode(z).cpu()
    h3 = tr.engine.act("h3", tail).cpu()
    r = {"h3": ck.check_gemm(h3, z, v["fc3.weight"].t(), v["fc3.bias"], relu=True)}
    t, bt = ck.gemm_ref(h3, v["fc4.weight"].t(), v["fc4.bias"])
    p = torch.sigmoid(t)
    r["recon"] = ck.ratio(out, p, bt / 4 + 8 * ck.U * p)
    _report(f"{sid} decode M={tail}", r)


IW_SHAPES = {"ragged": dict(B=48, tail=37, D=100, H=36, Z=12),
             # the largest H the pass's 64 KiB LDS decoder tile accepts
             "wide496": dict(B=32, tail=17, D=256, H=496, Z=32)}


@pytest.mark.parametrize("name", list(IW_SHAPES))
def test_iw_rows_match_float64_oracle(name, native_ext):
    from multidisttorch_amd.models.iw import iw_reduce, mlp_iw_log_weights
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
    from multidisttorch_amd.ops.philox import reparam_eps

    s = IW_SHAPES[name]
    B, Z, K = s["B"], s["Z"], 3
    n = B + s["tail"]
    X = torch.rand(n, s["D"], generator=torch.Generator().manual_seed(5)).to(_dev())
    tr = MlpVaeTrainer(batch_size=B, D=s["D"], H=s["H"], Z=Z, device=_dev(), backend="hip", seed=SEED,
                       use_graphs=False)
    r = tr.evaluate_iw(X, torch.arange(n, dtype=torch.int32, device=_dev()), K, chunk_samples=2, return_rows=True)
    torch.cuda.synchronize()
    v = {k: t.cpu().double() for k, t in tr.named_parameters().items()}
    rn, re_ = [], []
    for b in range(2):
        m = min(B, n - b * B)
        eps = torch.from_numpy(reparam_eps(K * B, Z, SEED, IW_STREAM, b).reshape(K, B, Z)[:, :m].copy()).double()
        logw, _ = mlp_iw_log_weights(v, X[b * B: b * B + m].cpu().double(), eps)
        a, e = iw_reduce(logw)
        rn.append(a)
        re_.append(e)
    rn, re_ = torch.cat(rn), torch.cat(re_)
    print(f"{name}: max rel err row_nll {float(((r['row_nll'].cpu().double() - rn).abs() / rn).max()):.3g} "
          f"row_neg_elbo {float(((r['row_neg_elbo'].cpu().double() - re_).abs() / re_).max()):.3g}")
    assert r["rows"] == n and r["k"] == K
    np.testing.assert_allclose(r["row_nll"].cpu().double().numpy(), rn.numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(r["row_neg_elbo"].cpu().double().numpy(), re_.numpy(), rtol=2e-5, atol=0)
    assert abs(r["nll"] - float(rn.sum())) <= 2e-5 * float(rn.sum())
    assert abs(r["neg_elbo"] - float(re_.sum())) <= 2e-5 * float(re_.sum())


# ------------------------------------------------------------ 5. the domain ----
@pytest.mark.parametrize("kw,msg", [
    (dict(Z=10), r"latent size Z = 10 must be a multiple of 4 in \[4, 32\]"),
    (dict(Z=36), r"latent size Z = 36 must be a multiple of 4 in \[4, 32\]"),
    (dict(H=402), r"hidden size H = 402 must be a positive multiple of 4"),
    (dict(H=516), r"hidden size H = 516 exceeds the limit of 512"),
    (dict(D=30), r"input size D = 30 must be a positive multiple of 4"),
    (dict(batch_size=4097), r"batch size 4097 must be in \[1, 4096\]"),
    (dict(D=16384, batch_size=512), r"batch size 512 with D = 16384 needs 131072 BCE partial slots .* limit 65536"),
])
def test_unsupported_shapes_fail_at_construction(kw, msg, native_ext):
    """Every shape mdt_vae_check would refuse at M = B is refused by the constructor,
    before anything is allocated or launched, with a message that names the limit."""
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    args = dict(batch_size=32, D=64, H=64, Z=8)
    args.update(kw)
    with pytest.raises(RuntimeError, match=msg):
        MlpVaeTrainer(device=_dev(), backend="hip", seed=SEED, use_graphs=False, **args)


def test_iw_pass_refuses_h_512_before_any_launch(native_ext):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    tr = MlpVaeTrainer(batch_size=16, D=32, H=512, Z=4, device=_dev(), backend="hip", seed=SEED, use_graphs=False)
    X = torch.rand(16, 32, device=_dev())
    before = tr.engine.act("h1", 16).clone()
    with pytest.raises(RuntimeError, match="H = 512 exceeds the importance-weighted pass's limit of 496"):
        tr.evaluate_iw(X, torch.arange(16, dtype=torch.int32, device=_dev()), 2)
    torch.cuda.synchronize()
    assert torch.equal(tr.engine.act("h1", 16), before), "the encoder ran before the shape was refused"
