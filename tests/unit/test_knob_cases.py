"""tests/knob_cases.py and the three checker extensions are not vacuous (CPU,
no GPU): with every objective knob of ``knob_cases.ALL`` in force at once, the
plain f32 emulations of the MLP step (tests/unit/test_mlp_checker.py) and of the
layer-path conv step (tests/unit/test_layer_checker.py) -- the penalty's share
folded into d[mu|lv] after the floor decision, Adam with the scheduled lr_t, the
decay and ``grad_scale``, the weight average after Adam, the eval forward on the
averaged weights -- pass every stage, the conditions on the inputs hold (floored
share, visible addend, no power without the addend, inside both ramps, average
below its cap), and each mutant fails at its own stage and at none before it."""
import math

import numpy as np
import pytest
import torch

from multidisttorch_amd.models.mlp_vae import arena_layout, init_params_, views
from multidisttorch_amd.ops.philox import reparam_eps
from tests import f28_checker as fk
from tests import free_bits_cases as fbc
from tests import knob_cases as kc
from tests import layer_checker as lk
from tests import mlp_checker as mk
from tests.unit import test_f28_checker as f28u
from tests.unit import test_layer_checker as lu
from tests.unit import test_mlp_checker as mu_

STREAM = 0


def _bad(r):
    return {k: (v if math.isinf(v) else round(v, 3)) for k, v in r.items() if not v <= 1}


def _flat(named, names):
    return torch.cat([named[n].float().reshape(-1) for n in names])


def _opt_state(P, names, seed=11):
    """Named moments (v >= m^2) and an average away from the parameters."""
    g = torch.Generator().manual_seed(seed)
    m, v, e = {}, {}, {}
    for n in names:
        m[n] = (torch.rand(P[n].numel(), generator=g) - 0.5) * 1e-2
        v[n] = m[n] ** 2 + torch.rand(P[n].numel(), generator=g) * 1e-4
        e[n] = P[n].float().reshape(-1) * (1.0 + 0.05 * torch.randn(P[n].numel(), generator=g))
    return m, v, e


def _adam_ema(P, grads, names, c, t, mut, m0, v0, e0):
    """f32 Adam and the average over named tensors -> flat (before, after, grads, e0, ema)."""
    from multidisttorch_amd.models.trainer_base import ema_omd

    after = dict(params=[], exp_avg=[], exp_avg_sq=[])
    ema = []
    for n in names:
        p = P[n].float().reshape(-1)
        p2, m2, v2 = lu._adam(p, grads[n].reshape(-1), m0[n], v0[n], c, mut)
        after["params"].append(p2), after["exp_avg"].append(m2), after["exp_avg_sq"].append(v2)
        omd = np.float32(ema_omd(kc.EMA_DECAY, t - (1 if mut == "ema_prev_d" else 0)))
        ema.append(e0[n] + omd * ((p if mut == "ema_pre_adam" else p2) - e0[n]))
    before = dict(params=_flat(P, names), exp_avg=_flat(m0, names), exp_avg_sq=_flat(v0, names))
    return before, {k: torch.cat(v) for k, v in after.items()}, _flat(grads, names), _flat(e0, names), torch.cat(ema)


def test_table_and_conditions():
    assert kc.ALL["schedule"].lr_warmup_steps == 8 and kc.ALL["schedule"].kl_anneal_steps == 16
    assert kc.ALL["schedule"].lr_decay == "cosine" and kc.ALL["schedule"].lr_decay_steps == 32
    assert (kc.KL_BETA, kc.TC_WEIGHT, kc.EMA_DECAY, kc.LR) == (0.5, 3.0, 0.9, 2e-3)
    assert kc.ADAM["decoupled"] == dict(weight_decay=0.01, decoupled_wd=True, grad_scale=1.0)
    assert kc.ADAM["coupled"] == dict(weight_decay=0.01, decoupled_wd=False, grad_scale=0.5)
    assert (kc.STEP0, kc.CURSOR0) == (4, 1)
    for t in kc.STEPS:
        kc.check_conditions(t)
        c = kc.adam_consts("decoupled", t)
        assert c["lr"] == kc.LR * t / 8 or abs(c["lr"] - kc.LR * t / 8) < 1e-18
    assert kc.effective(5) == dict(lr=kc.LR * 0.625, kl_beta=0.15625, tc_weight=0.9375, free_bits=0.0)


# --------------------------------------------------------------------- MLP ----
_MLP = {}


def _mlp_inputs(sid):
    if sid not in _MLP:
        s = mk.SHAPES[sid]
        layout, numel, _ = arena_layout(s["D"], s["H"], s["Z"])
        flat = torch.zeros(numel)
        init_params_(flat, layout, torch.Generator().manual_seed(kc.MLP_SEED))   # as MlpVaeTrainer(seed=3)
        v = {k: t.clone() for k, t in views(flat, layout).items()}
        kc.scale_mlp_heads(v)
        _MLP[sid] = (v, [n for n, _, _ in layout]) + kc.mlp_data(sid)
    return _MLP[sid]


def _mlp_run(sid, M, adam, mut=None, t=5):
    s = mk.SHAPES[sid]
    B, Z = s["B"], s["Z"]
    v, names, X, idx = _mlp_inputs(sid)
    cur = kc.cursor_of(t, kc.MLP_NBATCH)
    x = X[idx[cur * B: cur * B + M].long()]
    eps_np = reparam_eps(M, Z, kc.MLP_SEED, STREAM, t - 1)
    eps = torch.from_numpy(eps_np)
    eff = kc.effective(t)
    klw = eff["kl_beta"]
    d0, _, _ = mu_.emulate(v, x, eps, klw)
    kl = fbc.kl_elements(d0["mulv"], Z)
    fb = float(np.float32(fbc.choose_floor(kl)))
    mask, share = fbc.check_floor(kl, fb)
    kn = dict(tc_t=eff["tc_weight"], tc_weight=kc.TC_WEIGHT)
    d, g, loss = mu_.emulate(v, x, eps, klw, fb, mut, kn)
    tc, _ = kc.tc_of(d["mulv"], d["eps"], eff["tc_weight"])
    r = mk.check_forward(d, v, x, klw, eps_np, loss, fb)
    r.update(mk.check_backward(d, g, v, x, klw, fb, tc))
    c = kc.adam_consts(adam, t, kc.TORCH_OMB)
    c["lr0"] = kc.LR
    m0, v0, e0 = _opt_state(v, names)
    before, after, gflat, eflat, ema = _adam_ema(v, g, names, c, t, mut, m0, v0, e0)
    r.update(kc.check_adam(before, after, gflat, c))
    r.update(kc.check_ema(eflat, after["params"], ema, t))
    info = dict(d=d, g=g, v=v, x=x, klw=klw, fb=fb, tc=tc, mask=mask, share=share, Z=Z, eps_np=eps_np,
                names=names, after=after, ema=ema)
    return r, info


@pytest.mark.parametrize("adam", list(kc.ADAM))
@pytest.mark.parametrize("sid,M", kc.MLP_CASES)
def test_mlp_emulation_passes_and_meets_the_conditions(sid, M, adam):
    for t in kc.STEPS:
        r, i = _mlp_run(sid, M, adam, t=t)
        assert mk.first_failure(r) is None, _bad(r)
        assert set(k.split(".")[0] for k in r) == set(mk.STAGES)
        print(f"mlp {sid} M={M} t={t}: floor {i['fb']:.6g}, {i['share']:.3f} floored")
        d64 = {k: x.double() for k, x in i["d"].items()}
        W3 = i["v"]["fc3.weight"].double()
        kc.assert_visible(mk.dmulv_ref(d64, W3, i["klw"], i["fb"], i["tc"]), i["tc"], i["mask"], f"mlp {sid} M={M}")
        # no power without the addend: the same check with the addend left out of the reference fails
        none = (i["tc"][0], torch.zeros_like(i["tc"][1]), i["tc"][2])
        assert mk.check_backward(i["d"], i["g"], i["v"], i["x"], i["klw"], i["fb"], none)["dmulv"] > 1


# mutation -> (adam set, first failing stage of the MLP checker, of the layer checker)
MUTATIONS = {
    "fold_skips_floored": ("decoupled", "dmulv", "B.dec_fc"),
    "tc_no_ramp": ("decoupled", "dmulv", "B.dec_fc"),
    "consumer_prefold": ("decoupled", "dh1", "B.enc_head"),
    "wg_prefold": ("decoupled", "gfc21", "WG"),
    "floor_with_klt": ("decoupled", "loss", "F.reparam"),
    "decay_lr": ("decoupled", "AD", "AD"),
    "no_grad_scale": ("coupled", "AD", "AD"),
    "ema_pre_adam": ("coupled", "EM", "EM"),
    "ema_prev_d": ("coupled", "EM", "EM"),
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
@pytest.mark.parametrize("sid,M", [("tiny", 5), ("ragged", 37)])
def test_mlp_mutation_fails_at_its_own_stage(sid, M, mut):
    adam, want, _ = MUTATIONS[mut]
    r, _ = _mlp_run(sid, M, adam, mut)
    assert mk.first_failure(r) == want, (mut, _bad(r))


@pytest.mark.parametrize("mut,want", [(None, None), ("eval_raw_weights", "h1"), ("eval_keeps_floor", "loss")])
def test_mlp_eval_under_the_knobs(mut, want):
    """The eval pass inside averaged_weights(): the forward on the average, full kl_beta, no floor."""
    sid, M = "tiny", 5
    _, i = _mlp_run(sid, M, "coupled")
    names = i["names"]
    sizes = [i["v"][n].numel() for n in names]
    avg = {n: t.reshape(i["v"][n].shape) for n, t in zip(names, torch.split(i["ema"], sizes))}
    eps = torch.from_numpy(i["eps_np"])
    d, _, loss = mu_.emulate(i["v"] if mut == "eval_raw_weights" else avg, i["x"], eps, kc.KL_BETA,
                             i["fb"] if mut == "eval_keeps_floor" else 0.0)
    r = mk.check_forward(d, avg, i["x"], kc.KL_BETA, i["eps_np"], loss, 0.0)
    assert mk.first_failure(r) == want, (mut, _bad(r))


# ------------------------------------------------------------- layer path ----
LAYER_CASE = ("knobs", 28, 32, 16, 5, "knobs", "bin", kc.CURSOR0, kc.STEP0, {})
_LAYER = {}


def _layer_inputs():
    if not _LAYER:
        cid, image, z, B, M = LAYER_CASE[:5]
        base = lu._base(image, z)
        n = lk.data_rows(LAYER_CASE)
        _LAYER.update(spec=base["spec"], P=kc.conv_params(base["init"], base["spec"]),
                      X=lu._data("bin", image, n), idx=lk.make_idx(n))
    return _LAYER


def _layer_run(adam, mut=None, native=None):
    cid, image, z, B, M, _, _, cursor, step, _ = LAYER_CASE
    L = _layer_inputs()
    spec, P, X, idx = L["spec"], L["P"], L["X"], L["idx"]
    t = step + 1
    eff = kc.effective(t)
    klw = eff["kl_beta"]
    b0 = lu.emulate(spec, P, X, idx, B, M, cursor, step, klw)[0]
    kl = fbc.kl_elements(b0["mulv"], z)
    fb = float(np.float32(fbc.choose_floor(kl)))
    mask, share = fbc.check_floor(kl, fb)
    names = [l.name + s for l in spec for s in (".weight", ".bias")]
    m0, v0, e0 = _opt_state(P, names)
    c = kc.adam_consts(adam, t)
    c["lr0"] = kc.LR
    kn = dict(tc_t=eff["tc_weight"], tc_weight=kc.TC_WEIGHT, c=c, e0=e0, decay=kc.EMA_DECAY, t=t)
    b, grads, slabs, loss, after = lu.emulate(spec, P, X, idx, B, M, cursor, step, klw, fb, mut,
                                              opt=dict(exp_avg=m0, exp_avg_sq=v0), kn=kn)
    tc, _ = kc.tc_of(b["mulv"], b["eps"], eff["tc_weight"])
    rows = X[idx[cursor * B: cursor * B + M].long()]
    W = lk.weights_of(P, spec)
    pl = lk.plans(spec, M)
    r = lk.check_forward(spec, b, W, pl, rows, lu.SEED, lu.STREAM, step, fb)
    r.update(lk.check_backward(spec, b, W, pl, klw, fb, tc=tc))
    r.update(lk.check_grads(spec, b, pl, grads, slabs, loss, klw))
    before = dict(params={k: P[k].float().reshape(-1) for k in names}, exp_avg=m0, exp_avg_sq=v0)
    r.update(lk.check_adam(spec, before, after, grads, kc.adam_hp(adam), t))
    r.update(kc.check_ema(_flat(e0, names), _flat(after["params"], names), _flat(after["ema"], names), t))
    return r, dict(spec=spec, b=b, W=W, pl=pl, klw=klw, fb=fb, tc=tc, mask=mask, share=share, after=after, P=P,
                   rows=rows, names=names, X=X, idx=idx)


@pytest.mark.parametrize("adam", list(kc.ADAM))
def test_layer_emulation_passes_and_meets_the_conditions(adam, native_ext):
    r, i = _layer_run(adam)
    spec = i["spec"]
    assert lk.first_failure(spec, r) is None, _bad(r)
    assert set(lk.stage_of(k) for k in r) == set(lk.stages(spec)) | {"EM"}
    cond = lk.input_conditions(spec, i["b"], True)
    assert all(cond.values()), cond
    print(f"layer 28 z=32 M=5: floor {i['fb']:.6g}, {i['share']:.3f} floored")
    kc.assert_visible(lk.dmulv_ref(i["b"], i["klw"], i["fb"], i["tc"]), i["tc"], i["mask"], "layer 28 z=32 M=5")
    none = (i["tc"][0], torch.zeros_like(i["tc"][1]), i["tc"][2])
    assert lk.ratio(i["b"]["dmulv"], *lk.dmulv_ref(i["b"], i["klw"], i["fb"], none)) > 1


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_layer_mutation_fails_at_its_own_stage(mut, native_ext):
    adam, _, want = MUTATIONS[mut]
    r, i = _layer_run(adam, mut)
    assert lk.first_failure(i["spec"], r) == want, (mut, _bad(r))
    if mut == "wg_prefold":
        assert all(k.startswith("WG.enc_head.") for k in _bad(r)), _bad(r)


def test_layer_stale_bf16_copy_fails_the_twin_check_alone(native_ext):
    """dmulv16 left as rounded before the fold: the twin check catches it, and nothing else can -- every later
    stage is chained from the stored dmulv16. (A consumer that read the stale copy while the stored one is
    current is ``consumer_prefold`` / ``wg_prefold`` above.)"""
    r, i = _layer_run("decoupled", "dmulv16_prefold")
    assert set(_bad(r)) == {"B.dec_fc.dmulv16"}, _bad(r)


@pytest.mark.parametrize("mut,want", [(None, None), ("eval_raw_weights", "F.enc1"), ("eval_keeps_floor", "F.reparam")])
def test_layer_eval_under_the_knobs(mut, want, native_ext):
    cid, image, z, B, M, _, _, cursor, step, _ = LAYER_CASE
    _, i = _layer_run("coupled")
    spec, P = i["spec"], i["P"]
    avg = {n: i["after"]["ema"][n].reshape(P[n].shape) for n in i["names"]}
    b = lu.emulate(spec, P if mut == "eval_raw_weights" else avg, i["X"], i["idx"], B, M, cursor, step, kc.KL_BETA,
                   i["fb"] if mut == "eval_keeps_floor" else 0.0)[0]
    r = lk.check_forward(spec, b, lk.weights_of(avg, spec), i["pl"], i["rows"], lu.SEED, lu.STREAM, step, 0.0)
    assert lk.first_failure(spec, r) == want, (mut, _bad(r))


# ------------------------------------------------------ fused 28x28: AD, EM ----
@pytest.mark.parametrize("mut,adam,want", [(None, "decoupled", None), (None, "coupled", None),
                                           ("decay_lr", "decoupled", "AD"), ("no_grad_scale", "coupled", "AD"),
                                           ("ema_pre_adam", "decoupled", "EM"), ("ema_prev_d", "decoupled", "EM"),
                                           ("eval_keeps_floor", "coupled", "P4")])
def test_f28_adam_and_average_stages(mut, adam, want):
    """The AD and EM stages on the gradients of the fused step's emulation (no penalty on this form), and the
    eval forward that keeps the floor."""
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=8, image=28, device=torch.device("cpu"), backend="torch", seed=f28u.SEED)
    init = {k: v.detach().clone() for k, v in tr.named_parameters().items()}
    P = fk.spread_params(init)
    X, idx = fk.make_data("bin"), fk.make_idx()
    B, M, t = 8, 5, kc.STEPS[0]
    klw = kc.effective(t, tc=False)["kl_beta"]
    b0 = f28u.emulate(P, X, idx, B, M, kc.CURSOR0, kc.STEP0, klw)[0]
    kl = fbc.kl_elements(b0["mulv"], 32)
    fb = float(np.float32(fbc.choose_floor(kl)))
    fbc.check_floor(kl, fb)
    if mut == "eval_keeps_floor":
        b = f28u.emulate(P, X, idx, B, M, kc.CURSOR0, kc.STEP0, kc.KL_BETA, fb)[0]
        rows = X[idx[kc.CURSOR0 * B: kc.CURSOR0 * B + M].long()]
        r = fk.check_forward(b, fk.weights_of(P), rows, f28u.SEED, f28u.STREAM, kc.STEP0, 0.0)
        assert fk.first_failure(r) == want, _bad(r)
        return
    b, grads, slabs, loss = f28u.emulate(P, X, idx, B, M, kc.CURSOR0, kc.STEP0, klw, fb)
    names = list(grads)
    c = kc.adam_consts(adam, t)
    c["lr0"] = kc.LR
    m0, v0, e0 = _opt_state(P, names)
    before, after, gflat, eflat, ema = _adam_ema(P, grads, names, c, t, mut, m0, v0, e0)
    after["w16"] = after["params"].to(torch.bfloat16)
    r = kc.check_adam(before, after, gflat, c)
    r.update(kc.check_ema(eflat, after["params"], ema, t))
    assert set(fk.stage_of(k) for k in r) == set(fk.KNOB_STAGES)
    assert fk.first_failure(r) == want, (mut, _bad(r))
