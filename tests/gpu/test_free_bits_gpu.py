"""Free bits (``free_bits``, csrc/kernels/common.h: fb_fwd / fb_bwd) on one MI355X,
at every kernel site that forms the KL term: the fused 28x28 step (solo and
paired), the layer path at 28x28 (row and element-strided split-K combines) and
128x128, the stand-alone reparam kernels, and the MLP step.

Each case runs one step WITHOUT a floor (Adam skipped), reads the stored
``[mu | logvar]``, puts the floor in the widest gap of the middle of the
sorted float64 ``kl_d`` (tests/free_bits_cases.py), and runs the step again
with that floor from the same weights, rows and noise. The second run must
differ from the first in exactly the floored elements' KL gradients and in the
loss, and its encoder-side gradients must match the float64 oracle with the
kernels' bf16 rounding points (which the first run must miss: the power
condition). The path tests are bitwise comparisons at that floor.

The encoder heads are scaled up before the first step: at initialisation every
kl_d is ~1e-3 or less, formed in f32 from terms of size 1 (absolute error up to
~5e-7), which is the size of the gaps between neighbouring values there. Scaled,
the gaps are >= 1e-5 and the input condition below has room.
"""
import numpy as np
import pytest
import torch

from tests import free_bits_cases as fc
from tests import mlp_checker as ck

pytestmark = pytest.mark.gpu

BETA = 4.0
HEAD_SCALE = 4.0   # conv: enc_head.weight; the MLP's fc21 / fc22 take MLP_SCALE
MLP_SCALE = 6.0
ABS_GAP = 2e-6     # no kl_d within this of the floor (f32 rounding of kl_d is < 5e-7), besides 1e-4 * floor
SEEDS = (2, 3, 5)  # a seed whose inputs miss a condition is passed over (the conditions are on the inputs)


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


_data_cache = {}


def _data(rows, D, seed=7):
    key = (rows, D, seed)
    if key not in _data_cache:
        _data_cache.clear()
        X = torch.rand(rows, D, generator=torch.Generator().manual_seed(seed)).to(_dev())
        _data_cache[key] = (X, torch.arange(rows, device=_dev(), dtype=torch.int32))
    return _data_cache[key]


# ---------------------------------------------------------------- conv trainers
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
    """One step of M rows with the gradients left in the arena, then what it stored."""
    if tr.f28:
        tr.f28_skip_adam = True
        tr.train_steps(1, M=M)
    else:
        st, C = tr.state, tr.C
        C.step_begin(st.train_state, st.hparams)
        C.gather_rows(tr._data[0], tr._data[1], st.train_state, tr.B, M, tr.xb)
        tr._forward_hip(M, st.train_state, 0)
        tr._backward_hip(M, with_loss=True)
        tr._finalize_grads(M, False)
    torch.cuda.synchronize()
    assert not tr.f28 or int(tr.f28_err.item()) == 0
    return dict(mulv=tr.mulv[:M].clone(), eps=tr.eps[:M].clone(), z=tr.z16[:M].clone(), dmulv=tr.dmulv[:M].clone(),
                grads={k: v.clone() for k, v in tr.named_grads().items()},
                gacts={k: v.clone() for k, v in tr.gacts.items()}, loss=float(tr.loss_history()[0]),
                x=tr.xb[:M].clone())


def _pick(make, once, M, Z):
    """The first seed whose lambda = 0 step meets the input conditions ->
    (seed, that step's snapshot, float64 kl_d, floor, reference mask)."""
    why = []
    for seed in SEEDS:
        s0 = once(make(seed=seed), M)
        kl = fc.kl_elements(s0["mulv"], Z)
        fb = fc.choose_floor(kl)
        try:
            mask, share = fc.check_floor(kl, fb)
            assert float((kl - fb).abs().min()) > ABS_GAP, "an element within the f32 rounding of kl_d of the floor"
        except AssertionError as e:
            why.append(f"seed {seed}: {e}")
            continue
        print(f"seed {seed}: floor {fb:.6g}, {share:.3f} floored, nearest element {float((kl - fb).abs().min()):.3g} away")
        return seed, s0, kl, fb, mask
    raise AssertionError("no seed meets the input conditions: " + "; ".join(why))


def _check_latent(s0, s1, kl, fb, mask, Z):
    """What one step may and may not change when the floor is switched on."""
    for k in ("mulv", "eps", "z"):
        assert torch.equal(s0[k], s1[k]), k
    # the operands as the kernels hold them: mu, and sd = expf(0.5f * lv) as an f32 number (sd^2 - 1 cancels for
    # the floored elements, whose lv is small: a float64 sd would charge the kernel with expf's last bit)
    mu = s0["mulv"][:, :Z].double().cpu()
    sd = torch.exp(0.5 * s0["mulv"][:, Z:2 * Z]).double().cpu()
    d0, d1 = s0["dmulv"].double().cpu(), s1["dmulv"].double().cpu()
    dm0, dl0, dm1, dl1 = d0[:, :Z], d0[:, Z:], d1[:, :Z], d1[:, Z:]
    changed = (s0["dmulv"][:, :Z] != s1["dmulv"][:, :Z]).cpu() | (s0["dmulv"][:, Z:] != s1["dmulv"][:, Z:]).cpu()
    assert torch.equal(changed, mask), f"{int((changed != mask).sum())} elements floored otherwise than kl_d64 < floor"
    # floored elements lose exactly the KL part (fp32 rounding of the operands)
    tm = 1e-5 * (dm0.abs() + BETA * mu.abs())
    tl = 1e-5 * (dl0.abs() + 0.5 * BETA * (sd * sd - 1).abs())
    em = ((dm0 - dm1) - BETA * mu).abs()
    el = ((dl0 - dl1) - 0.5 * BETA * (sd * sd - 1)).abs()
    assert bool((em[mask] <= tm[mask]).all()), float((em[mask] / tm[mask]).max())
    assert bool((el[mask] <= tl[mask]).all()), float((el[mask] / tl[mask]).max())
    want = BETA * float((fb - kl[mask]).sum())
    got = s1["loss"] - s0["loss"]
    print(f"loss {s0['loss']:.4f} -> {s1['loss']:.4f}: + {got:.5f}, expected + {want:.5f}")
    assert want > 0 and abs(got - want) <= 1e-4 * abs(s1["loss"]), (got, want)


def _check_conv(s0, s1, tr1, oracle, tol, kl, fb, mask, Z):
    _check_latent(s0, s1, kl, fb, mask, Z)
    for k in s0["grads"]:
        if k.startswith("dec"):
            assert torch.equal(s0["grads"][k], s1["grads"][k]), k
    for k in s0["gacts"]:
        if k.startswith("dec"):
            assert torch.equal(s0["gacts"][k], s1["gacts"][k]), k
    loss, gref = oracle(tr1, s1["x"], s1["eps"], BETA, mask, fb)
    assert abs(s1["loss"] - loss) <= 1e-3 * abs(loss), (s1["loss"], loss)
    enc = [k for k in gref if k.startswith("enc")]
    errs = {k: _rel(s1["grads"][k], gref[k]) for k in enc}
    miss = _rel(s0["grads"]["enc_head.weight"], gref["enc_head.weight"])
    print("encoder grad rel-err vs the floored f64 oracle:", {k: round(v, 5) for k, v in errs.items()},
          f"| the step without a floor misses enc_head.weight by {miss:.4f} (needs > {3 * tol})")
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, bad
    assert miss > 3 * tol, miss


# ---------------------------------------------------------------- one step, every site
@pytest.mark.parametrize("M,pair", [(32, True), (13, True), (32, False), (13, False)])
def test_f28_step_floors_exactly_the_reference_set(M, pair, native_ext):
    def make(seed, **kw):
        tr = _conv(seed=seed, **kw)
        assert tr.f28
        tr.f28_pair = pair
        return tr

    seed, s0, kl, fb, mask = _pick(make, _conv_once, M, 32)
    tr = make(seed, free_bits=fb)
    s1 = _conv_once(tr, M)
    assert tr.read_state()["free_bits"] == float(np.float32(fb))
    _check_conv(s0, s1, tr, fc.emulated_f28, 1e-2, kl, fb, mask, 32)


@pytest.mark.parametrize("image,z,B,M", [(28, 32, 16, 16), (28, 32, 16, 13), (28, 24, 16, 13), (128, 64, 8, 8),
                                         (128, 64, 8, 5)])
def test_layer_path_floors_exactly_the_reference_set(image, z, B, M, native_ext, monkeypatch):
    """28x28 with MDT_CONV_F28=0 (Z = 32: the row combine; Z = 24: the
    element-strided one) and 128x128, Z = 64 (split-K head, row combine)."""
    monkeypatch.setenv("MDT_CONV_F28", "0")

    def make(seed, **kw):
        tr = _conv(image, z, B, seed=seed, **kw)
        assert not tr.f28
        return tr

    seed, s0, kl, fb, mask = _pick(make, _conv_once, M, z)
    tr = make(seed, free_bits=fb)
    s1 = _conv_once(tr, M)
    _check_conv(s0, s1, tr, fc.emulated_layer_path, 3e-2, kl, fb, mask, z)


def test_reparam_kernels_floor_the_reference_set(native_ext):
    """reparam / reparam_bwd (the head without split-K) on their own: the KLD
    partials and d[mu | logvar] from planted mulv, eps and dz, with a state
    (fb_t) and without one (HParams.free_bits)."""
    from multidisttorch_amd.ops import native

    C = native.require()
    M, Z = 37, 24
    g = torch.Generator().manual_seed(4)
    mulv = (torch.randn(M, 2 * Z, generator=g) * 0.4).to(_dev())
    dz = torch.randn(M, Z, generator=g).to(_dev())
    kl = fc.kl_elements(mulv, Z)
    fb = fc.choose_floor(kl)
    mask, _ = fc.check_floor(kl, fb)
    assert float((kl - fb).abs().min()) > ABS_GAP
    out = {}
    for lam in (0.0, fb):
        st = C.TrialState(0)
        st.set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, BETA, 1.0, 3, False, free_bits=lam)
        st.set_step(False, 1)
        eps, z16 = torch.zeros(M, Z, device=_dev()), torch.zeros(M, Z, device=_dev(), dtype=torch.bfloat16)
        part = torch.zeros((M * Z + 255) // 256, device=_dev())
        for name, state in (("train", st.train_state), ("eval", st.eval_state)):
            C.reparam(mulv, eps, z16, None, M, Z, state, st.hparams, 0, part)
            out[lam, name, "kld"] = float(part.double().sum())
        dm = {}
        for name, state in (("train", st.train_state), ("eval", st.eval_state), ("none", None)):
            dm[name] = torch.zeros(M, 2 * Z, device=_dev())
            C.reparam_bwd(dz, mulv, eps, dm[name], None, M, Z, st.hparams, state)
        torch.cuda.synchronize()
        out[lam, "eps"] = eps.clone()
        for name in dm:
            out[lam, name, "dmulv"] = dm[name].clone()
    # eval states never floor; no state reads HParams.free_bits
    for name in ("train", "eval", "none"):
        assert torch.equal(out[0.0, name, "dmulv"], out[0.0, "train", "dmulv"])
    assert torch.equal(out[fb, "eval", "dmulv"], out[0.0, "train", "dmulv"])
    assert torch.equal(out[fb, "none", "dmulv"], out[fb, "train", "dmulv"])
    assert out[fb, "eval", "kld"] == out[0.0, "train", "kld"] == out[0.0, "eval", "kld"]
    want = float(torch.where(mask, torch.full_like(kl, fb), kl).sum())
    assert abs(out[fb, "train", "kld"] - want) <= 1e-5 * want, (out[fb, "train", "kld"], want)
    assert abs(out[0.0, "train", "kld"] - float(kl.sum())) <= 1e-5 * float(kl.sum())
    d0, d1 = out[0.0, "train", "dmulv"], out[fb, "train", "dmulv"]
    changed = ((d0[:, :Z] != d1[:, :Z]) | (d0[:, Z:] != d1[:, Z:])).cpu()
    assert torch.equal(changed, mask)
    e = out[fb, "eps"].double().cpu()
    sd = torch.exp(0.5 * mulv[:, Z:].double().cpu())
    want_dl = 0.5 * dz.double().cpu() * e * sd
    assert torch.equal(d1[:, :Z].cpu()[mask], dz.cpu()[mask])  # dmu = dz exactly
    torch.testing.assert_close(d1[:, Z:].double().cpu()[mask], want_dl[mask], rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------- MLP
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


MLP_ACTS = ("h1", "mulv", "eps", "z", "h3", "recon", "dlog", "dh3", "dmulv", "dh1")


def _mlp_once(tr, M, fuse_adam=False):
    e = tr.engine
    v = {k: t.cpu().clone() for k, t in tr.named_parameters().items()}  # before a fused Adam moves them
    e.forward(tr._data[0], tr._data[1], M, True, False, 5, True)
    e.backward(tr._data[0], tr._data[1], M, 0, fuse_adam)
    torch.cuda.synchronize()
    s = {n: e.act(n, M).clone() for n in MLP_ACTS}
    s.update(grads={k: t.clone() for k, t in tr.named_grads().items()}, loss=float(tr.loss_history()[0]), v=v,
             x=e.act("xb", M).cpu().clone())
    return s


# default shape at B = 32 is not in the table: "wide" is the B = 32 shape (Z = 32, tail 17 there; 13 here),
# "ragged" has Z = 12 below the 16-wide latent tile, "tiny" Z = 4
@pytest.mark.parametrize("sid,M,fuse_adam", [("wide", 32, False), ("wide", 13, False), ("wide", 13, True),
                                             ("ragged", 37, False), ("tiny", 5, True)])
def test_mlp_step_floors_exactly_the_reference_set(sid, M, fuse_adam, native_ext):
    Z = ck.SHAPES[sid]["Z"]
    seed, s0, kl, fb, mask = _pick(lambda seed, **kw: _mlp(sid, seed, **kw), _mlp_once, M, Z)
    tr = _mlp(sid, seed, free_bits=fb)
    s1 = _mlp_once(tr, M, fuse_adam)
    assert tr.read_state()["free_bits"] == float(np.float32(fb))
    _check_latent(s0, s1, kl, fb, mask, Z)
    for n in ("h1", "h3", "recon", "dlog", "dh3"):
        assert torch.equal(s0[n], s1[n]), n
    for k in ("fc3.weight", "fc3.bias", "fc4.weight", "fc4.bias"):
        assert torch.equal(s0["grads"][k], s1["grads"][k]), k
    if fuse_adam:  # the same gradients as the step without Adam
        s2 = _mlp_once(_mlp(sid, seed, free_bits=fb), M, False)
        for k in s1["grads"]:
            assert torch.equal(s1["grads"][k], s2["grads"][k]), k
    # stage-wise float64 check (tests/mlp_checker.py bounds) with the KL weight zeroed on the reference set
    be = torch.where(mask, torch.zeros_like(kl), torch.full_like(kl, BETA))
    dev1 = {n: s1[n].cpu() for n in MLP_ACTS}
    r = ck.check_backward(dev1, {k: t.cpu() for k, t in s1["grads"].items()}, s1["v"], s1["x"], be)
    dev0 = {n: s0[n].cpu() for n in MLP_ACTS}
    miss = ck.check_backward(dev0, {k: t.cpu() for k, t in s0["grads"].items()}, s0["v"], s0["x"], be)["dmulv"]
    print(f"{sid} M={M}: worst error/bound per stage", {k: round(v, 3) for k, v in r.items()},
          f"| the step without a floor misses dmulv by {miss:.3g} bounds (needs > 3)")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    assert miss > 3.0, miss


# ---------------------------------------------------------------- path equivalence (bitwise)
_floors = {}


def _floor(kind):
    """A floor in the middle of the kind's step-0 kl_d values (as above)."""
    if kind not in _floors:
        if kind == "mlp":
            _, _, kl, fb, _ = _pick(lambda seed, **kw: _mlp("wide", seed, **kw), _mlp_once, 32, 32)
        elif kind == "c128":
            _, _, kl, fb, _ = _pick(lambda seed, **kw: _conv(128, 64, 8, seed=seed, **kw), _conv_once, 8, 64)
        else:
            _, _, kl, fb, _ = _pick(lambda seed, **kw: _conv(seed=seed, **kw), _conv_once, 32, 32)
        _floors[kind] = fb
    return _floors[kind]


def _make(kind, **kw):
    if kind == "mlp":
        return _mlp("wide", 2, **kw)
    if kind == "c128":
        return _conv(128, 64, 8, **kw)
    return _conv(**kw)


def _state_of(tr, steps):
    torch.cuda.synchronize()
    st = tr.read_state()
    assert st["step"] == steps
    h = tr.loss_history()[:steps].copy()
    assert np.isfinite(h).all()
    return h, tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), st


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4], (a[4], b[4])


@pytest.mark.parametrize("kind,tail", [("conv28", 13), ("c128", 5), ("mlp", 13)])
def test_eager_equals_graph_replay(kind, tail, native_ext):
    fb = _floor(kind)
    res = []
    for graphs in (False, True):
        tr = _make(kind, graphs=graphs, free_bits=fb)
        tr.train_steps(6)
        tr.train_steps(1, tail)
        res.append(_state_of(tr, 7))
        assert res[-1][4]["free_bits"] == float(np.float32(fb))
    _same(res[0], res[1])
    # and the floor is in force in both: a trainer without it ends elsewhere
    tr = _make(kind, graphs=True)
    tr.train_steps(6)
    tr.train_steps(1, tail)
    assert not torch.equal(_state_of(tr, 7)[1], res[0][1])


def test_f28_merged_paired_and_solo_forms_agree(native_ext):
    fb = _floor("conv28")
    res = []
    for merge, pair in ((False, False), (True, False), (True, True)):
        tr = _conv(free_bits=fb)
        tr.f28_merge, tr.f28_pair = merge, pair
        tr.train_steps(6)
        tr.train_steps(1, 13)
        res.append(_state_of(tr, 7) + (tr.dmulv.clone(),))
        assert int(tr.f28_err.item()) == 0
    for r in res[1:]:
        _same(res[0], r)
        assert torch.equal(res[0][5], r[5])


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_graph_picks_up_a_new_floor(kind, native_ext):
    fb = _floor(kind)
    g, e = _make(kind, graphs=True, free_bits=fb), _make(kind, free_bits=fb)
    for tr in (g, e):
        tr.train_steps(3)
        assert tr.read_state()["free_bits"] == float(np.float32(fb))
        tr.set_hparams(free_bits=2 * fb)
        tr.train_steps(3)
        assert tr.read_state()["free_bits"] == float(np.float32(2 * fb))
        tr.set_hparams(free_bits=0.0)
        tr.train_steps(3)
        assert tr.read_state()["free_bits"] == 0.0
    _same(_state_of(g, 9), _state_of(e, 9))
    # each change mattered: a trainer that kept the first floor ends elsewhere
    k = _make(kind, graphs=True, free_bits=fb)
    k.train_steps(9)
    assert not torch.equal(_state_of(k, 9)[1], g.params)


@pytest.mark.parametrize("kind", ["conv28", "mlp"])
def test_zero_floor_is_no_floor(kind, native_ext):
    a, b = _make(kind, graphs=True), _make(kind, graphs=True, free_bits=0.0)
    a.train_steps(6)
    b.train_steps(6)
    _same(_state_of(a, 6), _state_of(b, 6))
    assert a.read_state()["free_bits"] == 0.0


@pytest.mark.parametrize("kind", ["conv28", "c128", "mlp"])
def test_evaluate_reports_the_true_elbo(kind, native_ext):
    fb = _floor(kind)
    a, b = _make(kind, graphs=True, free_bits=fb), _make(kind, graphs=True)
    a.train_steps(3)
    b.load_state_dict(a.state_dict())
    X, idx = a._data[0], a._data[1]
    ev = idx[: 2 * a.B + 5]
    la, _ = a.evaluate(X, ev, want_first_recon=False)
    lb, _ = b.evaluate(X, ev, want_first_recon=False)
    assert la == lb and la == la and la > 0
    assert a.read_state(eval=True)["free_bits"] == 0.0 and a.read_state()["free_bits"] == float(np.float32(fb))
    np.testing.assert_array_equal(a.loss_history(eval=True)[:3], b.loss_history(eval=True)[:3])


def test_f28_trains_with_a_floor(native_ext):
    from multidisttorch_amd.data.datasets import synthetic_images
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    X = synthetic_images(2048, device=_dev())
    idx = torch.arange(2048, device=_dev(), dtype=torch.int32)
    tr = ConvVaeTrainer(batch_size=128, image=28, device=_dev(), backend="hip", seed=3, use_graphs=True, graph_steps=4,
                        free_bits=0.05)
    assert tr.f28
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 16)
    tr.train_steps(40)
    torch.cuda.synchronize()
    h = tr.loss_history()[:40]
    assert np.all(np.isfinite(h)) and h[-5:].mean() < 0.7 * h[:5].mean(), h
    assert int(tr.f28_err.item()) == 0 and tr.read_state()["step"] == 40
