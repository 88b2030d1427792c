"""Every training-step form with all objective knobs on at once, on one MI355X:
``knob_cases.ALL`` (lr warm-up + cosine decay, KL annealing, a free-bits floor,
the total-correlation penalty, weight averaging, binarized rows, coupled or
decoupled weight decay with ``grad_scale``) through the stage-by-stage checkers
(``mlp_checker``, ``layer_checker``, ``f28_checker``) with the three extensions
of tests/knob_cases.py: the penalty's share of d[mu|lv], the ``AD`` stage and
the ``EM`` stage. tests/unit/test_knob_cases.py shows them to be non-vacuous.

  MLP            tiny (M = 16, 5) and ragged (M = 37), both Adam sets: unfused
                 (forward, ``_tc_step``, ``backward(part=0)``) at t = 5, shipped
                 (``train_steps(1, M)``: Adam in the B3 epilogues, ``ema_update``)
                 at t = 5 and 6; tiny M = 5 with a one-rank reducer (``adam_flat``).
  layer path     28x28 z = 32 (row-form combine) B = 16, M = 5 and 16: manual,
                 shipped, shipped-2nd, decoupled; 28x28 z = 24 (element form)
                 M = 5, coupled; 128x128 z = 64 B = 8 M = 3: manual, shipped.
  fused 28x28    B = 8 M = 5 and B = 128 M = 77, no penalty (the form routes
                 away from it), both Adam sets, all four forms; ``AD`` on the
                 three deterministic ones: the step runs once with
                 ``f28_skip_adam`` (its gradient) and again from the same state
                 with Adam, and loss entry and mulv must agree bit for bit.

The floor is chosen from the same step without one (``free_bits_cases``); the
inputs must meet the conditions of the issue (floored share, distance from the
floor, a visible addend on the floored set, no power without the addend, inside
both ramps, the average below its cap), asserted here. Buffers are poisoned as
in the stage suites. Then: the eval pass under the knobs inside
``averaged_weights()``, graph replay against eager, and a mid-run change of
three knobs. Each check prints ``RATIO knobs.<form>.<stage> <error/bound>``; the
last test prints the largest ratio per stage and the module's wall time."""

import os
import socket
import time

import numpy as np
import pytest
import torch

from multidisttorch_amd.ops.philox import reparam_eps
from tests import f28_checker as fk
from tests import free_bits_cases as fbc
from tests import igemm_checker as ck
from tests import knob_cases as kc
from tests import layer_checker as lk
from tests import mlp_checker as mk
from tests.gpu import test_conv28_stages as fs
from tests.gpu import test_conv_layer_stages as ls

pytestmark = pytest.mark.gpu

SEEN = {}
T0 = time.time()


@pytest.fixture(autouse=True)
def _sync_after():
    t0 = time.time()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error is sticky: nothing more of this module can run after it
        pytest.exit(f"device error after a test of this module: {e}", returncode=3)
    print(f"WALL test {time.time() - t0:.2f} s")


def _dev():
    return torch.device("cuda", 0)


def _ok_all(form, ratios):
    bad = {}
    for k, r in ratios.items():
        name = ("layer" if form.startswith("layer") else form.split(".")[0]) + "." + k   # mlp | layer | f28 | eval
        SEEN[name] = max(SEEN.get(name, 0.0), r)
        print(f"RATIO knobs.{form}.{k} {r:.4g}")
        if not r <= 1:
            bad[k] = r
    assert not bad, (form, bad)


def _floor_of(mulv, Z):
    kl = fbc.kl_elements(mulv, Z)
    fb = float(np.float32(fbc.choose_floor(kl)))
    mask, share = fbc.check_floor(kl, fb)
    print(f"floor {fb:.6g}: {share:.3f} of the elements floored")
    return fb, mask


def _check_tc_value(rs, tc0, value, label):
    v64, bv = value
    ev = abs((rs["epoch_tc"] - tc0) - v64)
    print(f"RATIO knobs.{label}.epoch_tc {ev / bv:.4g}")
    assert ev <= bv, (rs["epoch_tc"], tc0, v64, bv)


# ======================================================================= MLP ====
_MLP_DATA = {}


def _mlp_data(sid):
    if sid not in _MLP_DATA:
        X, idx = kc.mlp_data(sid)
        _MLP_DATA[sid] = (X, idx, X.to(_dev()), idx.to(_dev()))
    return _MLP_DATA[sid]


def _mlp_trainer(sid, adam, fb=0.0, graphs=False, plant=True):
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    s = mk.SHAPES[sid]
    tr = MlpVaeTrainer(batch_size=s["B"], D=s["D"], H=s["H"], Z=s["Z"], device=_dev(), backend="hip",
                       seed=kc.MLP_SEED, use_graphs=graphs, graph_steps=3, **kc.trainer_kwargs(adam, fb=fb))
    kc.apply(tr, adam)
    kc.scale_mlp_heads(tr.named_parameters())
    _, _, X, idx = _mlp_data(sid)
    tr.bind_train_data(X, idx)
    tr.set_step(kc.STEP0)
    tr.set_cursor(kc.CURSOR0, kc.MLP_NBATCH)
    if plant:
        kc.plant_optimizer_state(tr)
    else:
        tr.reset_average()
    return tr


MLP_STORED = ("h1", "mulv", "eps", "z", "h3", "dlog", "dh3", "dmulv", "dh1")


def _mlp_step(tr, sid, M, adam, form, fb):
    """One step from the state the trainer holds -> ratios; ``form``: unfused | shipped."""
    s = mk.SHAPES[sid]
    B, Z = s["B"], s["Z"]
    Xc, idxc, X, idx = _mlp_data(sid)
    e = tr.engine
    rs0 = tr.read_state()
    step, cursor, t = rs0["step"], rs0["cursor"], rs0["step"] + 1
    assert cursor == kc.cursor_of(t, kc.MLP_NBATCH)
    v = {k: p.detach().cpu().clone() for k, p in tr.named_parameters().items()}
    before = dict(params=tr.params.clone(), exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone())
    e0 = tr.ema.clone()
    if form == "unfused":
        e.forward(X, idx, M, True, False, tr.rng_stream, True)
        tr._tc_step(M)
        e.backward(X, idx, M, 0, False)
    else:
        tr.train_steps(1, M)
    torch.cuda.synchronize()
    rs = tr.read_state()
    kc.assert_state(rs, t, True, fb)
    assert rs["cursor"] == (cursor + 1) % kc.MLP_NBATCH
    names = MLP_STORED + (("recon",) if form == "unfused" else ())
    dev = {n: e.act(n, M).cpu() for n in names}
    x = Xc[idxc[cursor * B: cursor * B + M].long()]
    assert torch.equal(e.act("xb", M).cpu(), x)
    if M < B:
        for n in names:
            assert not bool(e.act(n, B)[M:].any()), f"{n}: rows >= M written"
    used = kc._named_mask(tr).to(_dev())
    assert not bool(tr.grads[~used].any()), "padding of the gradient arena written"
    klw, fbk = rs["kl_beta"], rs["free_bits"]
    tc, value = kc.tc_of(dev["mulv"], dev["eps"], rs["tc_weight"])
    # the floor the kernels had to apply: no element of THIS step near it
    mask, _ = fbc.check_floor(fbc.kl_elements(dev["mulv"], Z), fbk)
    assert torch.equal(mk.floored_set(dev["mulv"], Z, fbk), mask)
    d64 = {k: a.double() for k, a in dev.items()}
    W3 = v["fc3.weight"].double()
    kc.assert_visible(mk.dmulv_ref(d64, W3, klw, fbk, tc), tc, mask, f"mlp {sid} M={M} t={t}")
    g = {k: a.cpu() for k, a in tr.named_grads().items()}
    loss = float(tr.loss_history()[step])   # BCE + kl_t KL with the floor, no penalty term
    r = mk.check_forward(dev, v, x, klw, reparam_eps(M, Z, tr.seed, tr.rng_stream, step), loss, fbk)
    r.update(mk.check_backward(dev, g, v, x, klw, fbk, tc))
    none = (tc[0], torch.zeros_like(tc[1]), tc[2])
    assert mk.ratio(d64["dmulv"], *mk.dmulv_ref(d64, W3, klw, fbk, none)) > 1, "no power without the addend"
    _check_tc_value(rs, rs0["epoch_tc"], value, f"mlp.{form}")
    if form == "unfused":
        for k, a in before.items():
            assert torch.equal(getattr(tr, k), a), k
        assert torch.equal(tr.ema, e0)
        want = set(mk.STAGES) - {"AD", "EM"}
    else:
        after = dict(params=tr.params, exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq)
        r.update(kc.check_adam(before, after, tr.grads, kc.adam_consts(adam, t, kc.TORCH_OMB)))
        r.update(kc.check_ema(e0, tr.params, tr.ema, t))
        for a in (tr.params, tr.exp_avg, tr.exp_avg_sq, tr.ema):
            assert not bool(a[~used].any()), "padding between arena tensors must stay zero"
        want = set(mk.STAGES) - {"recon"}
    assert set(k.split(".")[0] for k in r) == want, sorted(r)
    return r


def _mlp_floor(sid, M, adam):
    """The floor from the same step without one (its mulv depends on no knob)."""
    tr = _mlp_trainer(sid, adam)
    _, _, X, idx = _mlp_data(sid)
    tr.engine.forward(X, idx, M, True, False, tr.rng_stream, False)
    torch.cuda.synchronize()
    return _floor_of(tr.engine.act("mulv", M).cpu(), mk.SHAPES[sid]["Z"])[0]


@pytest.mark.parametrize("adam", list(kc.ADAM))
@pytest.mark.parametrize("sid,M", kc.MLP_CASES)
def test_mlp_unfused_and_shipped(sid, M, adam, native_ext):
    fb = _mlp_floor(sid, M, adam)
    _ok_all(f"mlp.unfused.{sid}.m{M}", _mlp_step(_mlp_trainer(sid, adam, fb), sid, M, adam, "unfused", fb))
    tr = _mlp_trainer(sid, adam, fb)
    for t in kc.STEPS:
        _ok_all(f"mlp.shipped.{sid}.m{M}.t{t}", _mlp_step(tr, sid, M, adam, "shipped", fb))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture()
def nccl_world():
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_mlp_with_a_one_rank_reducer(nccl_world, native_ext):
    """``adam_flat`` after the (identity) all-reduce instead of the B3 epilogues: nothing to wait for."""
    from multidisttorch_amd.parallel.ddp import make_arena_reducer

    sid, M, adam = "tiny", 5, "coupled"
    fb = _mlp_floor(sid, M, adam)
    tr = _mlp_trainer(sid, adam, fb)
    tr.attach_reducer(make_arena_reducer(nccl_world, tr.grads, tr.bucket_bounds(None)))
    try:
        for t in kc.STEPS:
            _ok_all(f"mlp.reducer.{sid}.m{M}.t{t}", _mlp_step(tr, sid, M, adam, "shipped", fb))
    finally:
        tr.attach_reducer(None)


# ================================================================ layer path ====
LAYER_FORMS = ("manual", "shipped", "shipped-2nd")
# (image, z, B, M, adam set, forms)
LAYER_CASES = [(28, 32, 16, 5, "decoupled", LAYER_FORMS), (28, 32, 16, 16, "decoupled", LAYER_FORMS),
               (28, 24, 16, 5, "coupled", LAYER_FORMS), (128, 64, 8, 3, "decoupled", ("manual", "shipped"))]


def _layer_trainer(image, z, B, adam, fb=0.0, graphs=False, tc=True, plant=True):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=B, image=image, z=z, device=_dev(), backend="hip", seed=kc.CONV_SEED,
                        use_graphs=graphs, graph_steps=3, **kc.trainer_kwargs(adam, tc=tc, fb=fb))
    kc.apply(tr, adam)
    init = {k: v.detach().cpu().clone() for k, v in tr.named_parameters().items()}
    new = kc.conv_params(init, tr.spec) if tc else fk.spread_params(init)
    with torch.no_grad():
        for k, v in new.items():
            tr.named_parameters()[k].copy_(v)
    tr.refresh_weights()
    n = lk.NBATCH * B
    _, _, X, idx = ls._data("bin", image, n, _dev())
    tr.bind_train_data(X, idx)
    tr.set_step(kc.STEP0)
    tr.set_cursor(kc.CURSOR0, lk.NBATCH)
    if plant:
        kc.plant_optimizer_state(tr)
    else:
        tr.reset_average()
    return tr


def _layer_step(tr, M, adam, form, fb):
    """One layer-path step from the state the trainer holds (tests/gpu/test_conv_layer_stages.py::_one_step with
    the knobs) -> (stored buffers, ratios)."""
    assert not tr.f28 and tr.tc_on and tr.ema_on
    spec, st, C, B = tr.spec, tr.state, tr.C, tr.B
    Xc, idxc, X, idx = ls._data("bin", tr.image, lk.NBATCH * B, _dev())
    p, pl = tr._plan(M), lk.plans(spec, M)
    rs0 = tr.read_state()
    step, cursor, t = rs0["step"], rs0["cursor"], rs0["step"] + 1
    W = ls._weights(tr)
    w16_0 = tr.w16.clone()
    before = dict(params=ls._named(tr, tr.params.clone()), exp_avg=ls._named(tr, tr.exp_avg.clone()),
                  exp_avg_sq=ls._named(tr, tr.exp_avg_sq.clone()))
    e0 = tr.ema.clone()
    ls._poison_all(tr, M)
    shipped = form != "manual"
    if shipped and tr._wt_deferred():
        for l in spec[1:]:
            ls._poison(tr._wt(l))
    ws_fwd = None
    if not shipped:
        C.step_begin(st.train_state, st.hparams)
        C.gather_rows(X, tr._data[1], st.train_state, B, M, tr.xb)
        tr._forward_hip(M, st.train_state, tr.rng_stream, want_recon=True)
        ws_fwd = p["ws"].clone()
        tr._backward_hip(M, with_loss=True)
        tr._finalize_grads(M, False)
        torch.cuda.synchronize()
    else:
        tr.train_steps(1, M=M)
        torch.cuda.synchronize()
        ls._check_wt(tr, w16_0 if tr._wt_deferred() else tr.w16)
        tr._ensure_wt()
        ls._check_wt(tr, tr.w16)
    rs = tr.read_state()
    kc.assert_state(rs, t, True, fb)
    assert rs["cursor"] == (cursor + 1) % lk.NBATCH
    klw, fbk = rs["kl_beta"], rs["free_bits"]
    b = ls._collect(tr, M, train=True, recon=not shipped)
    b["ws_fwd"] = ws_fwd
    after = None
    if shipped:
        after = dict(params=ls._named(tr, tr.params.clone()), exp_avg=ls._named(tr, tr.exp_avg.clone()),
                     exp_avg_sq=ls._named(tr, tr.exp_avg_sq.clone()), w16=ls._named(tr, tr.w16.clone()))
        p_after, e_after = tr.params.clone(), tr.ema.clone()
        tr._finalize_grads(M, False)   # the gradient the fused finalize + Adam consumed, from the same slabs
        torch.cuda.synchronize()
    else:
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert all(ck.same_bits(v, before[k][n]) for n, v in ls._named(tr, getattr(tr, k)).items()), k
        assert torch.equal(tr.ema, e0)
    grads = {k: v.detach().reshape(-1).clone() for k, v in tr.named_grads().items()}
    loss = float(tr.loss_history()[step])
    rows = Xc[idxc[cursor * B: cursor * B + M].long()]
    tc, value = kc.tc_of(b["mulv"], b["eps"], rs["tc_weight"])
    mask, _ = fbc.check_floor(fbc.kl_elements(b["mulv"], tr.Z), fbk)
    assert torch.equal(lk.floored_set(b["mulv"], fbk).cpu(), mask)
    kc.assert_visible(lk.dmulv_ref(b, klw, fbk, tc), tc, mask, f"layer {tr.image} z={tr.Z} M={M} t={t}")
    none = (tc[0], torch.zeros_like(tc[1]), tc[2])
    assert lk.ratio(b["dmulv"], *lk.dmulv_ref(b, klw, fbk, none)) > 1, "no power without the addend"
    r = lk.check_forward(spec, b, W, pl, rows, tr.seed, tr.rng_stream, step, fbk)
    r.update(lk.check_backward(spec, b, W, pl, klw, fbk, tc=tc))
    r.update(lk.check_grads(spec, b, pl, grads, p["slabs"], loss, klw))   # the loss: BCE + kl_t KL, no penalty term
    _check_tc_value(rs, rs0["epoch_tc"], value, f"layer.{form}")
    want = set(lk.stages(spec)) - {"AD"}
    if shipped:
        r.update(lk.check_adam(spec, before, after, grads, kc.adam_hp(adam), t))
        r.update(kc.check_ema(e0, p_after, e_after, t))
        want |= {"AD", "EM"}
    assert set(lk.stage_of(k) for k in r) == want, sorted(r)
    cond = lk.input_conditions(spec, b, True)
    assert all(cond.values()), cond
    return b, r


def _forward_floor(tr, M):
    """The floor for the step the trainer would run next, from a forward of that step (the trainer is spent)."""
    st, B, z = tr.state, tr.B, tr.Z
    tr.C.step_begin(st.train_state, st.hparams)
    tr.C.gather_rows(tr._data[0], tr._data[1], st.train_state, B, M, tr.xb)
    tr._forward_hip(M, st.train_state, tr.rng_stream)
    torch.cuda.synchronize()
    return _floor_of(tr.mulv[:M].cpu(), z)[0]


def _layer_floor(image, z, B, M, adam):
    return _forward_floor(_layer_trainer(image, z, B, adam), M)


@pytest.mark.parametrize("image,z,B,M,adam,forms", LAYER_CASES, ids=[f"{c[0]}-z{c[1]}-m{c[3]}" for c in LAYER_CASES])
def test_layer_path_with_every_knob(image, z, B, M, adam, forms, native_ext):
    fb = _layer_floor(image, z, B, M, adam)
    tag = f"layer{image}.z{z}.m{M}"
    for form in forms:
        t0 = time.time()
        tr = _layer_trainer(image, z, B, adam, fb)
        fbf = fb
        if form == "shipped-2nd":
            # one Adam step at this lr moves the 3136-wide head's outputs by O(1): the second step gets a floor
            # chosen for the mulv it will see (a twin trainer's forward after the same first step), set between
            # the steps -- free_bits is no structural knob
            twin = _layer_trainer(image, z, B, adam, fb)
            twin.train_steps(1, M=M)
            fbf = _forward_floor(twin, M)
            tr.train_steps(1, M=M)
            tr.set_hparams(free_bits=fbf)
        _, r = _layer_step(tr, M, adam, form, fbf)
        if form == "manual":
            assert "B.dec_fc.dmulv16" in r and "B.enc_head.gin" in r and "WG.enc_head.weight" in r
        print(f"WALL {tag} {form} {time.time() - t0:.2f} s")
        _ok_all(f"{tag}.{form}", r)


# =============================================================== fused 28x28 ====
def _f28_trainer(B, adam, fb=0.0, graphs=False, plant=True):
    tr = _layer_trainer(28, 32, B, adam, fb, graphs, tc=False, plant=plant)
    assert tr.f28 and not tr.tc_on and tr.ema_on
    _, _, X, idx = fs._data("bin", _dev())
    tr.bind_train_data(X, idx)       # f28_checker's 512 rows: NBATCH batches at B = 128
    tr.set_step(kc.STEP0)
    tr.set_cursor(kc.CURSOR0, fk.NBATCH)
    return tr


def _f28_step(B, M, adam, form, fb):
    from multidisttorch_amd.ops.conv_plans import wgrad_plan

    Xc, idxc, X, idx = fs._data("bin", _dev())
    tr = _f28_trainer(B, adam, fb)
    f = fs.FORMS[form]
    tr.f28_merge, tr.f28_pair, tr.f28_pair_delay_us = f["merge"], f["pair"], f["delay"]
    step, cursor, t = kc.STEP0, kc.CURSOR0, kc.STEP0 + 1
    W = fk.weights_from_list([w.clone() for w in tr._f28_weights()])
    plan = tr._plan28(M)
    st0 = tr.state.train_state.clone()
    before = dict(params=tr.params.clone(), exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone())
    e0 = tr.ema.clone()
    bufs = fs._buffers(tr)
    for a in bufs.values():
        fs._poison(a)
    fs._poison(tr.grads)
    for name in fk.WG_SHAPES:
        fs._poison(plan["slabs"][name + ".weight"][0])
    # 1. the gradient: the step without Adam
    tr.f28_skip_adam = True
    tr.train_steps(1, M=M)
    torch.cuda.synchronize()
    assert int(tr.f28_err.item()) == 0 and int(tr.f28_pairw.abs().sum()) == 0
    assert torch.equal(tr.params, before["params"])
    rs = tr.read_state()
    kc.assert_state(rs, t, False, fb)
    assert rs["cursor"] == (cursor + 1) % fk.NBATCH and rs["epoch_tc"] == 0.0
    klw, fbk = rs["kl_beta"], rs["free_bits"]
    b = fs._collect(bufs, M, fk.BUFS)
    mask, _ = fbc.check_floor(fbc.kl_elements(b["mulv"], 32), fbk)
    assert torch.equal(fk.floored_set(b["mulv"], fbk), mask)
    grads = {k: v.detach().cpu().clone() for k, v in tr.named_grads().items()}
    slabs = {}
    for name in fk.WG_SHAPES:
        a, ns = plan["slabs"][name + ".weight"]
        wp = wgrad_plan(tr._desc(tr.by_name[name], M))
        assert wp.nsplit == ns
        slabs[name] = (a.cpu(), ns, wp.mt_per_split)
    loss1 = tr.loss_history()[step].copy()
    rows = Xc[idxc[cursor * B: cursor * B + M].long()]
    r = fk.check_step(b, W, grads, slabs, float(loss1), rows, tr.seed, tr.rng_stream, step, klw, fbk)
    cond = fk.input_conditions(b, W, True, True)
    assert all(cond.values()), cond
    used = kc._named_mask(tr).to(_dev())
    assert ck.untouched(tr.grads[~used])   # the arena's padding: still the poison, never read
    G, mulv1 = torch.where(used, tr.grads, torch.zeros_like(tr.grads)), tr.mulv[:M].clone()
    # 2. the same step from the same state with Adam and the average
    tr.state.train_state.copy_(st0)
    tr.ema.copy_(e0)
    tr._invalidate_prefetch()
    tr.f28_skip_adam = False
    tr.train_steps(1, M=M)
    torch.cuda.synchronize()
    assert int(tr.f28_err.item()) == 0 and int(tr.f28_pairw.abs().sum()) == 0
    kc.assert_state(tr.read_state(), t, False, fb)
    want = set(fk.STAGES) | {"EM"}
    if form != "paired":   # which partner pairs is a race: the three other forms are deterministic
        assert tr.loss_history()[step].tobytes() == loss1.tobytes() and ck.same_bits(tr.mulv[:M], mulv1)
        after = dict(params=tr.params, exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq, w16=tr.w16)
        r.update(kc.check_adam(before, after, G, kc.adam_consts(adam, t)))
        want |= {"AD"}
    r.update(kc.check_ema(e0, tr.params, tr.ema, t))
    assert set(fk.stage_of(k) for k in r) == want, sorted(r)
    return r


_F28_FLOOR = {}


def _f28_floor(B, M, adam):
    if (B, M) not in _F28_FLOOR:
        tr = _f28_trainer(B, adam)
        tr.f28_skip_adam = True
        tr.train_steps(1, M=M)
        torch.cuda.synchronize()
        _F28_FLOOR[(B, M)] = _floor_of(tr.mulv[:M].cpu(), 32)[0]
    return _F28_FLOOR[(B, M)]


@pytest.mark.parametrize("form", list(fs.FORMS))
@pytest.mark.parametrize("adam", list(kc.ADAM))
@pytest.mark.parametrize("B,M", [(8, 5), (128, 77)])
def test_fused_28x28_with_every_knob_it_can_carry(B, M, adam, form, native_ext):
    fb = _f28_floor(B, M, adam)
    _ok_all(f"f28.b{B}.m{M}.{form}", _f28_step(B, M, adam, form, fb))


# ==================================================== eval under the knobs ====
def _derived(tr):
    return (tr.w16.clone(), tr.w16t.clone()) if hasattr(tr, "w16") else ()


def _eval_common(tr, M, nbatch, run_stage_checks):
    """Two steps, then inside averaged_weights(): the compute copies are the former average bit for bit, one
    ``_eval_batch`` through the forward stages, the eval state's effective values; afterwards everything is
    bitwise what it was, and ``evaluate()`` as hpo/runner.py calls it gives the same loss-ring entry."""
    X, idx = tr._data[0], tr._data[1]
    tr.train_steps(2, M)
    if hasattr(tr, "_ensure_wt"):
        tr._ensure_wt()
    torch.cuda.synchronize()
    p0, e0, d0 = tr.params.clone(), tr.ema.clone(), _derived(tr)
    assert not torch.equal(p0, e0)
    cursor, step = 1, 3
    with tr.averaged_weights():
        assert torch.equal(tr.params, e0) and torch.equal(tr.ema, p0)
        if d0:
            assert ck.twin_ok(tr.w16, e0)
            ls._check_wt(tr, tr.w16)
        tr.set_cursor(cursor, nbatch, eval=True)
        tr.state.set_step(True, step)
        r = run_stage_checks(cursor, step)
        rs = tr.read_state(eval=True)
        assert rs["step"] == step + 1 and rs["kl_beta"] == kc.KL_BETA and rs["free_bits"] == 0.0
        assert rs["tc_weight"] == 0.0
        entry = tr.loss_history(eval=True)[step].copy()
    torch.cuda.synchronize()
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, e0)
    for a, a0 in zip(_derived(tr), d0):
        assert torch.equal(a, a0), "w16 / w16t changed across the context"
    # the runner's call (hpo/runner.py::_test_epoch) on the same rows at the same eval step
    tr.state.set_step(True, step)
    with tr.averaged_weights():
        tr.evaluate(X, idx[cursor * tr.B: cursor * tr.B + M], want_first_recon=False)
    assert tr.loss_history(eval=True)[step].tobytes() == entry.tobytes()
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, e0)
    return r


def test_eval_under_the_knobs_mlp(native_ext):
    from multidisttorch_amd.models.trainer_base import EVAL_STREAM

    sid, M, adam = "tiny", 5, "coupled"
    s = mk.SHAPES[sid]
    Xc, idxc, X, idx = _mlp_data(sid)
    tr = _mlp_trainer(sid, adam, 0.4)

    def stages(cursor, step):
        v = {k: p.detach().cpu().clone() for k, p in tr.named_parameters().items()}   # the average
        tr._eval_batch(M, X, idx, True)
        torch.cuda.synchronize()
        dev = {n: tr.engine.act(n, M).cpu() for n in ("h1", "mulv", "eps", "z", "h3", "recon")}
        x = Xc[idxc[cursor * s["B"]: cursor * s["B"] + M].long()]
        loss = float(tr.loss_history(eval=True)[step])
        return mk.check_forward(dev, v, x, kc.KL_BETA, reparam_eps(M, s["Z"], tr.seed, EVAL_STREAM + tr.rng_stream, step),
                                loss, 0.0)

    r = _eval_common(tr, M, kc.MLP_NBATCH, stages)
    assert {"h1", "mulv", "eps", "z", "h3", "recon", "loss"} <= set(r)
    _ok_all("eval.mlp", r)


def test_eval_under_the_knobs_layer28(native_ext):
    from multidisttorch_amd.models.trainer_base import EVAL_STREAM

    image, z, B, M, adam = 28, 32, 16, 5, "decoupled"
    tr = _layer_trainer(image, z, B, adam, 0.2)
    Xc, idxc, X, idx = ls._data("bin", image, lk.NBATCH * B, _dev())

    def stages(cursor, step):
        W = ls._weights(tr)   # w16 is the twin of params, and params the average
        p = tr._plan(M)
        ls._poison_all(tr, M)
        tr._eval_batch(M, X, idx, True)
        torch.cuda.synchronize()
        b = ls._collect(tr, M, train=False, recon=True)
        b["ws_fwd"] = p["ws"]
        rows = Xc[idxc[cursor * B: cursor * B + M].long()]
        r = lk.check_forward(tr.spec, b, W, lk.plans(tr.spec, M), rows, tr.seed, EVAL_STREAM + tr.rng_stream, step, 0.0)
        bce, kld = b["bce_part"].double(), b["kld_part"].double()
        bound = (bce.numel() + kld.numel() + lk.SLACK) * lk.U * (bce.abs().sum() + kc.KL_BETA * kld.abs().sum())
        r["WG.loss"] = lk.ratio(torch.tensor(float(tr.loss_history(eval=True)[step]), dtype=torch.float64, device=_dev()),
                                bce.sum() + kc.KL_BETA * kld.sum(), bound)
        return r

    r = _eval_common(tr, M, lk.NBATCH, stages)
    assert "F.reparam.kld_part" in r and "F.enc1.act" in r
    _ok_all("eval.layer28", r)


def test_eval_under_the_knobs_f28(native_ext):
    """As tests/gpu/test_conv28_stages.py checks the eval pass: a forward launch that stores the chain, on the
    averaged weights, through every forward stage; then ``_eval_batch`` bit for bit against it."""
    from multidisttorch_amd.models.trainer_base import EVAL_STREAM

    B, M, adam = 8, 5, "coupled"
    tr = _f28_trainer(B, adam, 0.2)
    Xc, idxc, X, idx = fs._data("bin", _dev())

    def stages(cursor, step):
        st = tr.state
        # the weight list the launch reads: the f32 masters and w16 views of the exchanged arenas
        W = fk.weights_from_list(tr._f28_weights())
        Wp = fk.weights_of({k: v.detach().cpu() for k, v in tr.named_parameters().items()})
        for k in fk.W_ORDER:
            assert ck.same_bits(W[k].reshape(-1), Wp[k].reshape(-1)), k
        bufs = fs._buffers(tr)
        bufs["recon"] = tr.recon
        for a in bufs.values():
            fs._poison(a)
        table = tr._fwd_table28(X, idx, st.eval_state, True, recon=tr.recon)
        stream = EVAL_STREAM + tr.rng_stream
        tr.C.f28_forward(table, B, M, stream, True)
        torch.cuda.synchronize()
        b = fs._collect(bufs, M, fs.FWD_KEYS)
        assert ck.untouched(tr.recon.reshape(-1), M * 784)
        b["recon"] = tr.recon[:M * 784].cpu().reshape(M, 784)
        rows = Xc[idxc[cursor * B: cursor * B + M].long()]
        r = fk.check_forward(b, W, rows, tr.seed, stream, step, 0.0)   # no floor: kld_part is the true KL
        want = {k: bufs[k].reshape(-1)[:M * fk.BUFS.get(k, (784,))[0]].clone() for k in ("recon", "bce_part", "kld_part")}
        assert tr.read_state(eval=True)["step"] == step   # the bare launch advances nothing
        for k in want:
            fs._poison(bufs[k])
        tr._eval_batch(M, X, idx, True)
        torch.cuda.synchronize()
        assert int(tr.f28_err.item()) == 0 and int(tr.f28_pairw.abs().sum()) == 0
        for k, w in want.items():
            assert ck.same_bits(bufs[k].reshape(-1)[:w.numel()], w), k
        bce64, kld64 = b["bce_part"].double().reshape(M), b["kld_part"].double().reshape(M)
        bound = (M + fk.SLACK) * fk.U * (bce64.abs().sum() + kc.KL_BETA * kld64.abs().sum())
        r["WG.loss"] = fk.ratio(torch.tensor(float(tr.loss_history(eval=True)[step]), dtype=torch.float64),
                                bce64.sum() + kc.KL_BETA * kld64.sum(), bound)
        return r

    r = _eval_common(tr, M, fk.NBATCH, stages)
    assert {"P1.a1", "P4.kld_part", "P7.recon", "WG.loss"} <= set(r)
    _ok_all("eval.f28", r)


# ============================================== graph replay and mid-run change ====
def _make(kind, graphs, fb=0.3):
    if kind == "mlp":
        return _mlp_trainer("tiny", "coupled", fb, graphs, plant=False)
    if kind == "f28":
        return _f28_trainer(8, "coupled", fb, graphs, plant=False)
    if kind == "layer128":
        return _layer_trainer(128, 64, 8, "decoupled", fb, graphs, plant=False)
    return _layer_trainer(28, 32, 16, "decoupled", fb, graphs, plant=False)


def _state_of(tr, steps):
    torch.cuda.synchronize()
    rs = tr.read_state()
    assert rs["step"] == kc.STEP0 + steps
    h = tr.loss_history()[kc.STEP0: kc.STEP0 + steps].copy()
    assert np.isfinite(h).all() and np.isfinite(rs["epoch_tc"])
    return h, tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.ema.clone(), rs


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    for k, (x, y) in enumerate(zip(a[1:5], b[1:5])):
        assert torch.equal(x, y), ("params", "exp_avg", "exp_avg_sq", "ema")[k]
    assert a[5] == b[5], (a[5], b[5])


TAIL = {"mlp": 5, "f28": 5, "layer28": 13, "layer128": 5}


@pytest.mark.parametrize("kind", ["mlp", "f28", "layer28", "layer128"])
def test_graph_replay_equals_eager_with_every_knob(kind, native_ext):
    """2 graph_steps + 1 steps (t = 5 .. 11: through the end of the warm-up into the cosine decay), the last a
    tail batch: parameters, both moments, the average, the loss ring and read_state() bit for bit."""
    res = []
    for graphs in (False, True):
        tr = _make(kind, graphs)
        assert tr.use_graphs == graphs and tr.graph_steps == 3
        tr.train_steps(6)
        tr.train_steps(1, TAIL[kind])
        res.append(_state_of(tr, 7))
        rs = res[-1][5]
        # cos(pi p) on the host against cospi(p) on the device: equal up to the last bits of a double
        assert rs["kl_beta"] == kc.effective(11)["kl_beta"] and abs(rs["lr"] / kc.effective(11)["lr"] - 1) < 1e-12
        assert rs["lr"] < kc.LR and rs["free_bits"] == np.float32(0.3)
        assert (rs["tc_weight"] == kc.effective(11)["tc_weight"] and rs["epoch_tc"] != 0.0) if tr.tc_on else True
        if getattr(tr, "f28", False):
            assert int(tr.f28_err.item()) == 0
    _same(res[0], res[1])


@pytest.mark.parametrize("kind", ["mlp", "f28", "layer28"])
def test_mid_run_change_of_three_knobs(kind, native_ext):
    """After 3 steps ``set_hparams(tc_weight, free_bits, ema_decay)``: the captured graph picks the values up
    and ends bitwise where the eager run ends; a run without the change ends elsewhere."""
    res = []
    for graphs in (False, True):
        tr = _make(kind, graphs)
        tr.train_steps(3)
        new = dict(free_bits=0.05, ema_decay=0.25)
        if tr.tc_on:
            new["tc_weight"] = 0.5 * kc.TC_WEIGHT
        tr.set_hparams(**new)
        tr.train_steps(3)
        res.append(_state_of(tr, 6))
        rs = res[-1][5]
        assert rs["free_bits"] == np.float32(0.05)
        if tr.tc_on:
            assert rs["tc_weight"] == np.float32(np.float32(0.5 * kc.TC_WEIGHT) * 10 / 16)
    _same(res[0], res[1])
    k = _make(kind, True)
    k.train_steps(6)
    plain = _state_of(k, 6)
    assert not torch.equal(plain[1], res[0][1]) and not torch.equal(plain[4], res[0][4])
    np.testing.assert_array_equal(plain[0][:3], res[0][0][:3])   # the same run up to the change


def test_zz_report_largest_ratios():
    """Not a check of its own: prints the largest error/bound ratio each stage output reached in this run."""
    for name in sorted(SEEN):
        print(f"MAXRATIO knobs.{name} {SEEN[name]:.4g}")
    print(f"WALL module {time.time() - T0:.1f} s")
