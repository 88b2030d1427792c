"""tests/layer_checker.py is not vacuous (CPU, no GPU): a plain torch f32
emulation of the layer-path conv-VAE step -- every buffer, split-K slab, bias
partial row and weight-gradient slab the kernels store, in the kernels'
layouts, with bf16 stores at the kernels' rounding points -- passes every stage
check at ratio <= 1 on every small case, each mutated emulation fails at the
stage its mutation belongs to and at no stage before it, and the case table
covers every kernel choice the planner makes for the shipped batches."""
import math

import numpy as np
import pytest
import torch

from multidisttorch_amd.models.conv_spec import conv_vae_spec
from tests import conv_small_checker as sk
from tests import direct_checker as dc
from tests import free_bits_cases as fbc
from tests import igemm_checker as ck
from tests import layer_checker as lk

BF = torch.bfloat16
SEED, STREAM = 2, 0
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, decoupled=False,
          lr_warmup_steps=0)


# ---------------------------------------------------------------- emulation ----
def _bf(t, trunc=False):
    """The bf16 store of an f32 tensor: to nearest even, or (mutation) truncated."""
    if trunc:
        t = (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return t.to(BF)


def _sums(v, own, rows):
    return lk.owner_sums(v, own, rows)


def _block_sums(v, owners):
    v = v.reshape(-1)
    return torch.stack([v[o].sum() for o in owners])


def _adam(p, g, m, v, c, mut=None):
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    gr = g * f(1.0 if mut == "no_grad_scale" else c["gs"])
    if c["wd"] != 0:
        if c["decoupled"]:   # the decay uses the step's lr_t (mutation: the unscheduled lr)
            p = p * (1 - f(c["lr0"] if mut == "decay_lr" else c["lr"]) * f(c["wd"]))
        else:
            gr = gr + f(c["wd"]) * p
    # adam_update's two fmaf: the product of two f32 numbers is exact in float64, so one rounding each
    m2 = (m.double() + f(c["omb1"]).double() * (gr - m).double()).float()
    v2 = ((f(c["b2"]) * v).double() + f(c["omb2"]).double() * (gr * gr).double()).float()
    den = v2.sqrt() / f(c["bc2s"]) + f(c["eps"])
    return p - f(c["step_size"]) * m2 / den, m2, v2


def emulate(spec, P, X, idx, B, M, cursor, step, klw=1.0, fb=0.0, mut=None, opt=None, stale=None, kn=None):
    """One step in f32 -> (buffers, grads, slabs, loss, after). ``mut`` names one mutation (MUTATIONS, or
    those of tests/unit/test_knob_cases.py); ``opt``: named exp_avg / exp_avg_sq (zeros when None); ``stale``:
    weights of an earlier step that the ``stale_dec`` mutation lets dec1 read. ``kn``: the other knobs of
    tests/knob_cases.py -- tc_t and tc_weight (the penalty's share, folded into d[mu|lv] after the
    reparameterisation backward, dmulv16 rewritten), c (Adam's constants, with lr0 the unscheduled lr), e0,
    decay and t (the weight average, after Adam)."""
    from multidisttorch_amd.ops.philox import reparam_eps
    from tests import tc_cases as tcc

    kn = kn or {}

    pl = lk.plans(spec, M)
    W = lk.weights_of(P, spec)
    n = len(spec)
    Z = spec[n // 2].cin
    b = dict(acts={}, gacts={}, colsum={})
    nob = lambda name: 0.0 if mut == "nobias_" + name else 1.0
    rows = X[idx[cursor * B: cursor * B + M].long()].float()
    b["xb"] = rows.clone()
    pre_act = {}
    # ---- forward
    h = rows
    for i, l in enumerate(spec):
        N, H, C, CO, k, s, p = sh = lk.shape_of(l, M)
        OH = (H + 2 * p - k) // s + 1
        w, bias = W[l.name]["w"].float(), W[l.name]["b"]
        if mut == "stale_dec" and l.name == "dec1":
            w = stale[l.name]["w"].float()
        if mut == "khkw_swap" and l.name == "dec1":
            w = w.transpose(1, 2)
        q = pl[l.name]["F"]
        if l.name == "enc_head":
            a, wm = h.float().reshape(M, -1), w.reshape(CO, -1)
            if q.ksplit > 1:
                kps = -(-q.ktiles // q.ksplit)
                sl = [a[:, 64 * t:64 * (t + kps)] @ wm[:, 64 * t:64 * (t + kps)].T for t in range(0, q.ktiles, kps)]
                b["ws_fwd"] = torch.stack(sl).reshape(-1)
                b["mulv"] = torch.stack(sl).sum(0) + nob(l.name) * bias
            else:
                b["mulv"] = a @ wm.T + nob(l.name) * bias
            mu, lv = b["mulv"][:, :Z], b["mulv"][:, Z:]
            b["eps"] = torch.from_numpy(reparam_eps(M, Z, SEED, STREAM, step + (1 if mut == "philox_step" else 0)))
            sd = torch.exp(0.5 * lv)
            b["z16"] = _bf(mu + b["eps"] * sd)
            ksum = 1 + lv - mu * mu - sd * sd
            kl_f = np.float32(klw) * (-0.5 * ksum) if mut == "floor_with_klt" else -0.5 * ksum
            fl = (kl_f < fb) if fb > 0 else torch.zeros_like(ksum, dtype=torch.bool)
            term = -0.5 * torch.where(fl, torch.full_like(ksum, -2 * fb), ksum)
            b["kld_part"] = _block_sums(term, sk.block_owners(M, Z, q.ksplit if q.ksplit > 1 else None))
            h = b["z16"]
            continue
        if l.kind == "convT":
            pre = ck.tconv_ref(h.float().reshape(M, OH, OH, CO), w, s, p, H) + nob(l.name) * bias
        else:
            x = h.float() if i else rows
            pre = ck.im2col(x.reshape(M, H, H, C), k, s, p) @ w.reshape(CO, -1).T + nob(l.name) * bias
        if i == n - 1:
            t = pre.reshape(M, -1)
            x = rows
            pr = torch.sigmoid(t)
            sp = torch.relu(t) + torch.log1p(torch.exp(-t.abs()))
            loss = x * torch.clamp(sp - t, max=100.0) + (1 - x) * torch.clamp(sp, max=100.0)
            g32 = pr - x
            b["dlog16"], b["recon"], b["logits"] = _bf(g32), pr, t
            owners = dc.tconv_owners(CO, (M, H, H))
            b["bce_part"], b["gpart"] = _block_sums(loss, owners), _block_sums(g32, owners)
            continue
        pre_act[l.name] = torch.relu(pre)
        b["acts"][l.name] = _bf(torch.relu(pre), trunc=(mut == "trunc_store" and l.name == "enc2"))
        h = b["acts"][l.name]
    # ---- backward
    g = b["dlog16"]
    for i in range(n - 1, 0, -1):
        l, prev = spec[i], spec[i - 1]
        N, H, C, CO, k, s, p = sh = lk.shape_of(l, M)
        OH = (H + 2 * p - k) // s + 1
        w = W[l.name]["w"].float()
        q = pl[l.name]["D"]
        if l.name == "dec_fc":
            gm, wm = g.float().reshape(M, -1), w.reshape(-1, Z)
            if q.ksplit > 1:
                kps = -(-q.ktiles // q.ksplit)
                sl = torch.stack([gm[:, 64 * t:64 * (t + kps)] @ wm[64 * t:64 * (t + kps)]
                                  for t in range(0, q.ktiles, kps)])
                b["ws_bwd"], b["dz"] = sl.reshape(-1), sl.sum(0)
            else:
                b["dz"] = gm @ wm
            dz = b["dz"]
            be = torch.where(fl, torch.zeros_like(dz), torch.full_like(dz, 1.0 if mut == "kl_weight" else klw))
            b["dmulv"] = torch.cat([dz + be * mu, 0.5 * dz * b["eps"] * sd + 0.5 * be * (sd * sd - 1)], 1)
            pre16 = _bf(b["dmulv"])
            if kn.get("tc_t"):
                tct = kn["tc_weight"] if mut == "tc_no_ramp" else kn["tc_t"]
                add = np.float32(tct) * tcc.oracle(b["mulv"], b["eps"], torch.float32)[1].float()
                if mut == "fold_skips_floored":
                    add = add * (~torch.cat([fl, fl], 1))
                b["dmulv"] = b["dmulv"] + add
            b["dmulv16"] = pre16 if mut == "dmulv16_prefold" else _bf(b["dmulv"])
            src = b["dmulv"] if mut == "lin_bias_f32" else b["dmulv16"].float()
            b["colsum"]["enc_head"] = _rows8(src)
            g = pre16 if mut == "consumer_prefold" else b["dmulv16"]
            continue
        if q == "thin":
            v = ck.im2col(g.float().reshape(M, H, H, 1), 4, 2, 1) @ w.reshape(CO, 16).T
            mode, qq = 0, -(-v.shape[0] // 256)
        elif l.kind == "convT":
            v = ck.im2col(g.float().reshape(M, H, H, C), k, s, p) @ w.reshape(CO, -1).T
            mode, qq = 0, q
        else:
            v = ck.tconv_ref(g.float().reshape(M, OH, OH, CO), w, s, p, H)
            mode, qq = 1, q
        if prev.relu:
            act = pre_act[prev.name] if (mut == "mask_pre" and i == n - 1) else b["acts"][prev.name].float()
            v = v * (act.reshape(v.shape) > 0)
        b["gacts"][prev.name] = _bf(v)
        if prev.name == "dec_fc":
            b["colsum"][prev.name] = _rows8(b["gacts"][prev.name].float().reshape(M, -1))
        else:
            own, nr = lk.colsum_owner(qq, sh, mode)
            vv = v
            if mut == "parity_class" and l.name == "enc2":
                vv = v.clone()
                vv[ck.parity_rows(sh, 3)] = 0
            b["colsum"][prev.name] = _sums(vv, own, nr).reshape(-1)
        g = b["gacts"][prev.name]
    # ---- weight gradients and finalize
    grads, slabs = {}, {}
    brows = lk.bias_rows(spec, M, pl)
    for i, l in enumerate(spec):
        N, H, C, CO, k, s, p = sh = lk.shape_of(l, M)
        wp = pl[l.name]["W"]
        src = i
        if mut == "wg_pair" and l.name == "dec1":   # the mirror encoder layer's pair: same conv-view geometry
            src = [j for j, m in enumerate(spec) if m.name == "enc2"][0]
        G, Xw = lk.wg_pair(spec, src, b)
        if mut == "wg_prefold" and l.name == "enc_head":
            G = pre16.reshape(G.shape)
        xf = Xw.float() if wp.cfg == 110 else Xw.to(BF).float()
        cols = ck.im2col(xf, k, s, p)
        Gm = G.float().reshape(-1, CO)
        step_rows = lk.wg_rows_per_slab(wp, sh)
        sl = torch.stack([(Gm[r:r + step_rows].T @ cols[r:r + step_rows]).reshape(-1)
                          for r in range(0, Gm.shape[0], step_rows)])
        assert sl.shape[0] == wp.nsplit, (l.name, sl.shape, wp)
        use = sl[:-1] if (mut == "last_slab" and l.name == "enc2") else sl
        grads[l.name + ".weight"] = use.sum(0)
        if wp.nsplit > 1:
            slabs[l.name + ".weight"] = (sl.reshape(-1), wp.nsplit)
        part = b["gpart"] if i == n - 1 else b["colsum"][l.name]
        slabs[l.name + ".bias"] = (part, brows[l.name])
        grads[l.name + ".bias"] = part.reshape(brows[l.name], l.cout).sum(0)
    total = float(b["bce_part"].sum() + np.float32(klw) * b["kld_part"].sum())
    # ---- Adam
    c = kn["c"] if "c" in kn else sk.adam_consts(HP, step + (2 if mut == "adam_step" else 1))
    after = dict(params={}, exp_avg={}, exp_avg_sq={}, w16={}, ema={})
    for name, gr in grads.items():
        m0 = opt["exp_avg"][name] if opt else torch.zeros_like(gr)
        v0 = opt["exp_avg_sq"][name] if opt else torch.zeros_like(gr)
        p2, m2, v2 = _adam(P[name].float().reshape(-1), gr, m0.reshape(-1), v0.reshape(-1), c, mut)
        after["params"][name], after["exp_avg"][name], after["exp_avg_sq"][name] = p2, m2, v2
        after["w16"][name] = p2.to(BF)
        if "e0" in kn:   # e + (1 - d_t) (p - e) from the parameters Adam just wrote, at the step it advanced to
            from multidisttorch_amd.models.trainer_base import ema_omd

            e0 = kn["e0"][name].float().reshape(-1)
            omd = np.float32(ema_omd(kn["decay"], kn["t"] - (1 if mut == "ema_prev_d" else 0)))
            after["ema"][name] = e0 + omd * ((P[name].float().reshape(-1) if mut == "ema_pre_adam" else p2) - e0)
    return b, grads, slabs, total, after


def _rows8(v):
    M, N = v.shape
    r = -(-M // lk.ROWS_PER)
    pad = torch.zeros((r * lk.ROWS_PER, N))
    pad[:M] = v
    return pad.view(r, lk.ROWS_PER, N).sum(1).reshape(-1)


# mutation -> the stage that must be the first to fail (28x28, z = 32)
MUTATIONS = {
    "nobias_enc1": "F.enc1", "nobias_enc2": "F.enc2", "nobias_enc_head": "F.enc_head", "nobias_dec_fc": "F.dec_fc",
    "nobias_dec1": "F.dec1", "nobias_dec2": "F.dec2",
    "trunc_store": "F.enc2", "khkw_swap": "F.dec1", "philox_step": "F.reparam",
    "mask_pre": "B.dec2", "parity_class": "B.enc2", "lin_bias_f32": "B.dec_fc", "kl_weight": "B.dec_fc",
    "wg_pair": "WG", "last_slab": "WG", "adam_step": "AD",
}


# -------------------------------------------------------------------- inputs ----
_BASE = {}


def _base(image, z):
    if (image, z) not in _BASE:
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

        tr = ConvVaeTrainer(batch_size=8, image=image, z=z, device=torch.device("cpu"), backend="torch", seed=SEED)
        init = {k: v.detach().clone() for k, v in tr.named_parameters().items()}
        spec = conv_vae_spec(image, 1, z)
        _BASE[(image, z)] = dict(spec=spec, init=init, spread=lk.spread_params(init, spec))
    return _BASE[(image, z)]


_DATA = {}


def _data(kind, image, n):
    if (kind, image, n) not in _DATA:
        _DATA[(kind, image, n)] = lk.make_data(kind, image, n)
    return _DATA[(kind, image, n)]


def _klw(step, knobs):
    if "kl_beta" in knobs:
        return float(np.float32(knobs["kl_beta"] * min(1.0, (step + 1) / knobs["kl_anneal_steps"])))
    return 1.0


def _check(spec, b, P, grads, slabs, loss, after, rows, step, klw, fb, before=None):
    W = lk.weights_of(P, spec)
    M = b["xb"].shape[0]
    pl = lk.plans(spec, M)
    r = lk.check_forward(spec, b, W, pl, rows, SEED, STREAM, step, fb)
    r.update(lk.check_backward(spec, b, W, pl, klw, fb))
    r.update(lk.check_grads(spec, b, pl, grads, slabs, loss, klw))
    if before is None:
        zeros = {k: torch.zeros_like(v.reshape(-1)) for k, v in grads.items()}
        before = dict(params={k: P[k].float().reshape(-1) for k in grads}, exp_avg=zeros, exp_avg_sq=zeros)
    r.update(lk.check_adam(spec, before, after, grads, HP, step + 1))
    return r


def _run(case, mut=None, P=None):
    cid, image, z, B, M, pset, data, cursor, step, knobs = case
    base = _base(image, z)
    spec = base["spec"]
    P = base[pset] if P is None else P
    n = lk.data_rows(case)
    X, idx = _data(data, image, n), lk.make_idx(n)
    klw, fb = _klw(step, knobs), 0.0
    if knobs.get("free_bits"):
        b0 = emulate(spec, P, X, idx, B, M, cursor, step, klw)[0]
        kl = fbc.kl_elements(b0["mulv"], z)
        fb = float(np.float32(fbc.choose_floor(kl)))
        fbc.check_floor(kl, fb)
    b, grads, slabs, loss, after = emulate(spec, P, X, idx, B, M, cursor, step, klw, fb, mut)
    rows = X[idx[cursor * B: cursor * B + M].long()]
    return spec, b, _check(spec, b, P, grads, slabs, loss, after, rows, step, klw, fb)


def _bad(r):
    return {k: (v if math.isinf(v) else round(v, 3)) for k, v in r.items() if not v <= 1}


# --------------------------------------------------------------------- tests ----
SMALL = [c for c in lk.CASES if c[0] in lk.SMALL]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_emulation_passes_every_stage_and_meets_the_input_conditions(case, native_ext):
    spec, b, ratios = _run(case)
    assert not _bad(ratios), _bad(ratios)
    assert set(lk.stage_of(k) for k in ratios) == set(lk.stages(spec))
    cond = lk.input_conditions(spec, b, case[5] == "spread")
    assert all(cond.values()), cond


def test_case_table_covers_every_planner_choice_of_the_shipped_batches(native_ext):
    """Every (layer, direction, cfg, ksplit > 1, nsplit > 1, finalize rp > 1) of a shipped batch occurs in some
    case: a planner change that moves a shipped layer to an unchecked kernel fails here."""
    have = lk.case_tuples()
    small = lk.case_tuples([c for c in lk.CASES if c[1] == 128])
    big = lk.plan_tuples(*lk.BIG[1:3], lk.BIG[4])
    for image, z, B in lk.SHIPPED:
        need = lk.plan_tuples(image, z, B)
        missing = need - have - (big if (image, z, B) == (128, 64, 64) else set())
        assert not missing, (image, z, B, sorted(missing, key=str))
    # what the B = 64 case adds over the small 128x128 cases, and so what the GPU test checks of it
    extra = big - small
    assert {t[1] for t in extra if t[2] == "D"} == set(lk.BIG_ONLY["backward"]), extra
    assert {t[1] for t in extra if t[2] in "WB"} == set(lk.BIG_ONLY["grads"]), extra
    assert not [t for t in extra if t[2] == "F"], extra
    assert ("enc4", "D", 5) in {t[1:4] for t in extra}


def test_cases_are_what_the_gpu_test_needs():
    ids = {c[0] for c in lk.CASES}
    assert set(lk.SMALL) <= ids
    assert {c[4] for c in lk.CASES if c[1] == 128} == {1, 3, 8}
    assert {c[4] for c in lk.CASES if c[1] == 28 and c[2] == 32 and c[3] == 16} >= {1, 5, 16}
    assert {c[2] for c in lk.CASES if c[1] == 28 and c[4] == 5} >= {8, 24, 32, 128}
    assert {c[4] for c in lk.CASES if c[3] == 128} == {77, 128}
    assert {c[6] for c in lk.CASES} == {"rand", "mnist", "bin"} and {c[5] for c in lk.CASES} == {"init", "spread"}
    assert any(c[7] and c[8] for c in lk.CASES)
    kl = [c for c in lk.CASES if "kl_beta" in c[9]]
    assert kl and all(c[9]["kl_anneal_steps"] > c[8] + 1 for c in kl)
    assert any(c[9].get("free_bits") for c in lk.CASES)
    for c in lk.CASES:
        assert c[7] < lk.NBATCH and c[4] <= c[3]


def test_data_sets_are_what_they_claim():
    for image in (28, 128):
        m, bn = lk.make_data("mnist", image, 16), lk.make_data("bin", image, 16)
        img = m.view(-1, image, image)
        e = image // 7
        assert float(img[:, :e].abs().max()) == 0 and float(img[:, :, -e:].abs().max()) == 0
        assert bool((m == 1.0).any()) and bool(((m > 0) & (m < 1)).any())
        assert set(bn.unique().tolist()) == {0.0, 1.0}


# the case the mutations run on: small, spread parameters, exact zeros in x, cursor and step live, a KL weight
# that is not 1 and a floor
MUT_CASE = ("mut", 28, 32, 16, 5, "spread", "mnist", 2, 5, {"kl_beta": 0.5, "kl_anneal_steps": 16, "free_bits": True})


def _underflow_params(P):
    """dec1 scaled so that its pre-activations are f32 subnormals around the smallest bf16 subnormal: a positive
    value below 2^-134 is stored as 0, and only then do the mask of the value before rounding and the mask of
    the stored activation differ."""
    Q = {k: v.clone() for k, v in P.items()}
    Q["dec1.weight"] = Q["dec1.weight"] * 1e-41
    Q["dec1.bias"] = Q["dec1.bias"] * 1e-41
    return Q


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_fails_at_its_own_stage(mut, native_ext):
    P = _underflow_params(_base(28, 32)["spread"]) if mut == "mask_pre" else None
    if P is not None:  # the planted case itself passes unmutated
        spec, _, clean = _run(MUT_CASE, None, P)
        assert lk.first_failure(spec, clean) is None, _bad(clean)
    spec, _, ratios = _run(MUT_CASE, mut, P)
    assert lk.first_failure(spec, ratios) == MUTATIONS[mut], (mut, _bad(ratios))


def test_mutation_case_is_clean(native_ext):
    spec, _, ratios = _run(MUT_CASE)
    assert lk.first_failure(spec, ratios) is None, _bad(ratios)


def test_second_step_decoder_on_the_first_steps_weights_fails_at_that_layer(native_ext):
    """Two emulated steps: the second is checked against the weights the first one's Adam left. A decoder layer
    that still reads the weights of before the first step (a transposed copy never rewritten) fails at its own
    forward stage; the honest second step passes everywhere."""
    cid, image, z, B, M, pset, data, cursor, step, knobs = lk.CASES[4]
    base = _base(image, z)
    spec, P0 = base["spec"], base[pset]
    n = lk.data_rows(lk.CASES[4])
    X, idx = _data(data, image, n), lk.make_idx(n)
    _, _, _, _, a1 = emulate(spec, P0, X, idx, B, M, cursor, step)
    P1 = {k: v.reshape(P0[k].shape) for k, v in a1["params"].items()}
    opt = dict(exp_avg=a1["exp_avg"], exp_avg_sq=a1["exp_avg_sq"])
    cur2 = (cursor + 1) % lk.NBATCH
    rows = X[idx[cur2 * B: cur2 * B + M].long()]
    before = dict(params={k: v.reshape(-1) for k, v in P1.items()}, **opt)
    for mut, want in ((None, None), ("stale_dec", "F.dec1")):
        b, grads, slabs, loss, a2 = emulate(spec, P1, X, idx, B, M, cur2, step + 1, mut=mut, opt=opt,
                                            stale=lk.weights_of(P0, spec))
        r = _check(spec, b, P1, grads, slabs, loss, a2, rows, step + 1, 1.0, 0.0, before)
        assert lk.first_failure(spec, r) == want, (mut, _bad(r))
