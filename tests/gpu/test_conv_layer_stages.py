"""The layer-by-layer conv-VAE step (models/conv_layers.py over conv_igemm.hip,
conv_direct.h, conv_thin.hip, conv_small.h, conv_jobs.hip) per element and
stage by stage on one MI355X, against the chained float64 oracles and derived
bounds of tests/layer_checker.py (``lk``), which tests/unit/
test_layer_checker.py shows to be non-vacuous.

Every case of ``lk.CASES`` (128x128 z = 64 at B = 8 with M = 1, 3, 8; 28x28 with
MDT_CONV_F28=0 at B = 16 with z = 32 and M = 1, 5, 16, z = 8, 24, 128 at M = 5,
and B = 128 with M = 77, 128; the initial and the ``spread`` parameters;
uniform / MNIST-like / binarized rows; cursor and step != 0; a KL weight on its
ramp; a free-bits floor) runs on four forms:

  manual         step_begin, gather_rows, _forward_hip, a copy of the split-K
                 workspace, _backward_hip(with_loss), _finalize_grads: all stages;
  jobs-off       the same with MDT_CONV_JOBS=0 (every op its own kernel);
  shipped        train_steps(1, M): the gather in the first conv, fused jobs,
                 finalize + Adam spread over the backward launches, deferred
                 transposes at 28x28: every stage that survives the step
                 (not the head's forward slabs), plus the Adam stage;
  shipped-2nd    two steps; the second is checked with the weights the first
                 left (w16 == bf16(params) bitwise, the transposed copies
                 parity_transpose(w16) after _ensure_wt).

Before the checked step every output buffer is poisoned over its whole
allocation (NaN, or BF16_FILL for bf16; slabs, partial rows and the workspace
included); afterwards rows >= M of every per-sample buffer must still hold the
poison. ``lk.BIG`` (128x128, B = M = 64) checks only the stages whose planner
tuple no small case has. The eval and decode tests check ``_eval_batch`` and
``decode()``. Each check prints ``RATIO layer.<stage>.<output> <error/bound>``;
the last test prints the largest ratio per output. Oracles run in float64 on
the device."""

import time

import numpy as np
import pytest
import torch

from multidisttorch_amd.ops.conv_layout import parity_transpose
from tests import free_bits_cases as fbc
from tests import igemm_checker as ck
from tests import layer_checker as lk

pytestmark = pytest.mark.gpu

SEED = 2
SEEN = {}
FORMS = ("manual", "jobs-off", "shipped", "shipped-2nd")
_DATA = {}
T0 = time.time()


@pytest.fixture(autouse=True)
def _layer_path(monkeypatch):
    monkeypatch.setenv("MDT_CONV_F28", "0")
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error is sticky: nothing more of this module can run after it
        pytest.exit(f"device error after a test of this module: {e}", returncode=3)


def _ok_all(prefix, ratios):
    bad = {}
    for k, r in ratios.items():
        name = prefix + k
        SEEN[k] = max(SEEN.get(k, 0.0), r)
        print(f"RATIO layer.{name} {r:.4g}")
        if not r <= 1:
            bad[name] = r
    assert not bad, bad


def _data(kind, image, n, dev):
    key = (kind, image, n)
    if key not in _DATA:
        X, idx = lk.make_data(kind, image, n), lk.make_idx(n)
        _DATA[key] = (X, idx, X.to(dev), idx.to(dev))
    return _DATA[key]


def _trainer(case, fb=0.0):
    from multidisttorch_amd.hpo.schedule import Schedule
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    cid, image, z, B, M, pset, data, cursor, step, knobs = case
    kw = {}
    if "kl_beta" in knobs:
        kw = dict(kl_beta=knobs["kl_beta"], schedule=Schedule(kl_anneal_steps=knobs["kl_anneal_steps"]))
    tr = ConvVaeTrainer(batch_size=B, image=image, z=z, device=torch.device("cuda"), backend="hip", seed=SEED,
                        use_graphs=False, free_bits=fb, **kw)
    assert not tr.f28 and (tr._thin_first, tr._thin_last) == lk.thin_edges(tr.spec)
    if pset == "spread":
        init = {k: v.detach().cpu().clone() for k, v in tr.named_parameters().items()}
        with torch.no_grad():
            for k, v in lk.spread_params(init, tr.spec).items():
                tr.named_parameters()[k].copy_(v)
        tr.refresh_weights()
    return tr


def _bufs(tr):
    """name -> (tensor over the whole allocation, elements per sample) of every per-sample output of the step."""
    Z, D = tr.Z, tr.D
    t = {"xb": (tr.xb, D), "mulv": (tr.mulv, 2 * Z), "eps": (tr.eps, Z), "z16": (tr.z16, Z), "dz": (tr.dz, Z),
         "dmulv": (tr.dmulv, 2 * Z), "dmulv16": (tr.dmulv16, 2 * Z), "dlog16": (tr.dlog16, D), "recon": (tr.recon, D),
         "logits": (tr.logits, D)}
    for l in tr.spec[:-1]:
        per = l.out_hw * l.out_hw * l.cout
        t["act." + l.name] = (tr.acts[l.name], per)
        if l.name != "enc_head":
            t["gact." + l.name] = (tr.gacts[l.name], per)
    return t


def _poison(t):
    t.fill_(float("nan") if t.dtype == torch.float32 else lk.BF16_FILL)


def _poison_all(tr, M):
    p = tr._plan(M)
    for t, _ in _bufs(tr).values():
        _poison(t)
    for t in (tr.bce_part, tr.kld_part, tr.grads, p["ws"], p["gpart"]):
        _poison(t)
    for t in p["colsum"].values():
        _poison(t)
    for t, _ in p["slabs"].values():
        _poison(t)


FWD = {"xb", "mulv", "eps", "z16"}
BWD = {"dz", "dmulv", "dmulv16", "dlog16"}


def _collect(tr, M, train=True, recon=False):
    """The first M rows of every buffer the step wrote (on the device), and that every later row -- and every
    buffer the form does not write -- still holds the poison."""
    spec, p = tr.spec, tr._plan(M)
    wrote = set(FWD) | {"act." + l.name for l in spec[:-1] if l.name != "enc_head"}
    if train:
        wrote |= BWD | {"gact." + l.name for l in spec[:-1] if l.name != "enc_head"}
    if recon:
        wrote.add("recon")
    got, late = {}, []
    for k, (t, per) in _bufs(tr).items():
        n = M * per if k in wrote else 0
        if not ck.untouched(t.reshape(-1), n):
            late.append(k)
        got[k] = t.reshape(-1)[:n].reshape(M, per) if n else None
    nb, nk = tr._n_bce(M), tr._n_kld(M)
    for k, t, n in (("bce_part", tr.bce_part, nb), ("kld_part", tr.kld_part, nk)):
        if not ck.untouched(t.reshape(-1), n):
            late.append(k)
    assert not late, f"rows >= {M} (or a buffer this form does not write) were written: {late}"
    b = dict(xb=got["xb"], mulv=got["mulv"], eps=got["eps"], z16=got["z16"], dz=got["dz"], dmulv=got["dmulv"],
             dmulv16=got["dmulv16"], dlog16=got["dlog16"], recon=got["recon"],
             acts={l.name: got["act." + l.name] for l in spec[:-1] if l.name != "enc_head"},
             gacts={l.name: got["gact." + l.name] for l in spec[:-1] if l.name != "enc_head"} if train else {},
             bce_part=tr.bce_part[:nb], kld_part=tr.kld_part[:nk], gpart=p["gpart"] if train else None,
             colsum=p["colsum"], ws_bwd=p["ws"])
    for l in spec[:-1]:
        if l.name != "enc_head":
            b["acts"][l.name] = b["acts"][l.name].reshape(-1, l.cout)
            if train:
                b["gacts"][l.name] = b["gacts"][l.name].reshape(-1, l.cout)
    return b


def _named(tr, arena):
    from multidisttorch_amd.models.trainer_base import views

    return {k: v.reshape(-1) for k, v in views(arena, tr.layout).items()}


def _weights(tr):
    """The weights as the step's kernels read them (clones: the step updates them), after checking that w16 is
    the bf16 rounding of params bit for bit."""
    assert ck.twin_ok(tr.w16, tr.params)
    P = {k: v.detach().clone() for k, v in tr.named_parameters().items()}
    return lk.weights_of(P, tr.spec)


def _check_wt(tr, w16):
    """The transposed copies of layers 1.. are the parity transposes of ``w16`` (a flat bf16 arena)."""
    from multidisttorch_amd.models.conv_spec import _w_shape

    for l in tr.spec[1:]:
        o, s = tr._param_at[l.name + ".weight"]
        w = w16.narrow(0, o, int(np.prod(s))).view(_w_shape(l))
        assert ck.same_bits(tr._wt(l), parity_transpose(w, l.s)), l.name


def _one_step(case, form, monkeypatch, fb=0.0, only=None):
    """One step of the case on the form -> (trainer, stored buffers, ratios)."""
    cid, image, z, B, M, pset, data, cursor, step, knobs = case
    dev = torch.device("cuda")
    if form == "jobs-off":
        monkeypatch.setenv("MDT_CONV_JOBS", "0")
    Xc, idxc, X, idx = _data(data, image, lk.data_rows(case), dev)
    tr = _trainer(case, fb)
    assert tr.fuse_jobs == (form != "jobs-off")
    spec, st, C = tr.spec, tr.state, tr.C
    tr.bind_train_data(X, idx)
    tr.set_step(step)
    tr.set_cursor(cursor, lk.NBATCH)
    p = tr._plan(M)
    pl = lk.plans(spec, M)
    if form == "shipped-2nd":
        tr.train_steps(1, M=M)
        step, cursor = step + 1, (cursor + 1) % lk.NBATCH
    W = _weights(tr)
    w16_0 = tr.w16.clone()
    before = dict(params=_named(tr, tr.params.clone()), exp_avg=_named(tr, tr.exp_avg.clone()),
                  exp_avg_sq=_named(tr, tr.exp_avg_sq.clone()))
    _poison_all(tr, M)
    if form.startswith("shipped") and tr._wt_deferred():
        for l in spec[1:]:      # the step itself writes the transposed copies it reads
            _poison(tr._wt(l))
    ws_fwd = None
    if form in ("manual", "jobs-off"):
        C.step_begin(st.train_state, st.hparams)
        C.gather_rows(X, tr._data[1], st.train_state, tr.B, M, tr.xb)
        tr._forward_hip(M, st.train_state, tr.rng_stream, want_recon=True)
        ws_fwd = p["ws"].clone()
        tr._backward_hip(M, with_loss=True)
        tr._finalize_grads(M, False)
        torch.cuda.synchronize()
    else:
        tr.train_steps(1, M=M)
        torch.cuda.synchronize()
        # the transposed copies: written inside the step from the weights it ran on where they are deferred
        # (28x28), from the updated weights in the optimizer tail elsewhere; current after _ensure_wt
        _check_wt(tr, w16_0 if tr._wt_deferred() else tr.w16)
        assert tr._wt_stale == tr._wt_deferred()
        tr._ensure_wt()
        _check_wt(tr, tr.w16)
    rs = tr.read_state()
    assert rs["step"] == step + 1 and rs["cursor"] == (cursor + 1) % lk.NBATCH
    klw, fbk = rs["kl_beta"], rs["free_bits"]
    if "kl_beta" in knobs:
        want = float(np.float32(knobs["kl_beta"] * (step + 1) / knobs["kl_anneal_steps"]))
        assert klw == want and 0 < klw < knobs["kl_beta"], (klw, want)
    else:
        assert klw == 1.0
    assert fbk == float(np.float32(fb))
    shipped = form.startswith("shipped")
    b = _collect(tr, M, train=True, recon=not shipped)
    b["ws_fwd"] = ws_fwd
    after = None
    if shipped:
        after = dict(params=_named(tr, tr.params.clone()), exp_avg=_named(tr, tr.exp_avg.clone()),
                     exp_avg_sq=_named(tr, tr.exp_avg_sq.clone()), w16=_named(tr, tr.w16.clone()))
        # the gradient the fused finalize + Adam consumed in registers: the same kernel without Adam, from the
        # same stored slabs (nsplit = 1 segments hold it already)
        tr._finalize_grads(M, False)
        torch.cuda.synchronize()
    else:
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert all(ck.same_bits(v, before[k][n]) for n, v in _named(tr, getattr(tr, k)).items()), k
    grads = {k: v.detach().reshape(-1).clone() for k, v in tr.named_grads().items()}
    loss = float(tr.loss_history()[step])
    rows = Xc[idxc[cursor * B: cursor * B + M].long()]
    if only is not None:
        r = lk.check_backward(spec, b, W, pl, klw, fbk, only=only["backward"])
        r.update(lk.check_grads(spec, b, pl, grads, p["slabs"], None, klw, only=only["grads"]))
        return tr, b, r
    r = lk.check_forward(spec, b, W, pl, rows, tr.seed, tr.rng_stream, step, fbk)
    r.update(lk.check_backward(spec, b, W, pl, klw, fbk))
    r.update(lk.check_grads(spec, b, pl, grads, p["slabs"], loss, klw))
    if shipped:
        hp = lk.adam_hp(tr.hp, tr.decoupled_wd, tr.schedule)
        r.update(lk.check_adam(spec, before, after, grads, hp, step + 1))
    return tr, b, r


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", lk.CASES, ids=[c[0] for c in lk.CASES])
def test_every_stage_of_the_layer_path_step_within_its_bound(case, form, native_ext, monkeypatch):
    t0 = time.time()
    fb = 0.0
    if case[9].get("free_bits"):
        # the floor comes from the step without one: the midpoint of the widest gap of its kl_d values, with
        # every element away from it, so the kernels must floor exactly the float64 set
        _, b0, _ = _one_step(case, form, monkeypatch)
        kl = fbc.kl_elements(b0["mulv"], case[2])
        fb = float(np.float32(fbc.choose_floor(kl)))
        mask, share = fbc.check_floor(kl, fb)
        print(f"floor {fb:.6g}: {share:.3f} of the elements floored")
    tr, b, ratios = _one_step(case, form, monkeypatch, fb)
    cond = lk.input_conditions(tr.spec, b, case[5] == "spread")
    assert all(cond.values()), cond
    if fb:
        # the set the kernels had to floor: no element of THIS step near the floor either (the second step of
        # shipped-2nd follows a first step that already ran with the floor, so its mulv is not b0's)
        mask2, _ = fbc.check_floor(fbc.kl_elements(b["mulv"], case[2]), fb)
        assert torch.equal(lk.floored_set(b["mulv"], fb).cpu(), mask2)
        assert form == "shipped-2nd" or torch.equal(mask2, mask)
    want = set(lk.stages(tr.spec)) - (set() if form.startswith("shipped") else {"AD"})
    assert set(lk.stage_of(k) for k in ratios) == want
    if form == "manual":
        assert "F.enc_head.slabs" in ratios and "B.dec_fc.slabs" in ratios
    print(f"WALL {case[0]} {form} {time.time() - t0:.2f} s")
    _ok_all("", ratios)


def test_shipped_batch_of_128x128_stages_no_small_case_reaches(native_ext, monkeypatch):
    """B = M = 64: enc4's backward-data on another tile, and the finalize forms with more than 16 per-image slabs
    (enc2, dec3) and more than one colsum-kernel row (the Linear biases). Everything else of this batch runs
    the kernels the small cases check (tests/unit/test_layer_checker.py)."""
    t0 = time.time()
    tr, b, ratios = _one_step(lk.BIG, "manual", monkeypatch, only=lk.BIG_ONLY)
    assert {"B.enc4.gin", "B.enc4.colsum", "WG.enc2.weight", "WG.dec3.weight", "WG.enc_head.bias",
            "WG.dec_fc.bias"} <= set(ratios)
    print(f"WALL {lk.BIG[0]} manual {time.time() - t0:.2f} s")
    _ok_all("b64.", ratios)


@pytest.mark.parametrize("cid", ["128-m3-spread-mnist", "28-m5-spread-mnist", "28-z24-m5"])
def test_eval_batch_forward_stages_and_recon(cid, native_ext, monkeypatch):
    """``_eval_batch`` (train = False, want_recon = True): every forward stage and recon on the eval state and
    stream; dlog16, the bias partials and everything of the backward stay untouched, and so does the
    training state."""
    from multidisttorch_amd.models.trainer_base import EVAL_STREAM

    case = next(c for c in lk.CASES if c[0] == cid)
    cid, image, z, B, M, pset, data, cursor, step, knobs = case
    dev = torch.device("cuda")
    Xc, idxc, X, idx = _data(data, image, lk.data_rows(case), dev)
    tr = _trainer(case)
    tr.bind_train_data(X, idx)
    tr.set_cursor(cursor, lk.NBATCH, eval=True)
    tr.state.set_step(True, step)
    tr._ensure_wt()
    train0 = tr.read_state()
    arenas = [t.clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq, tr.w16, tr.w16t)]
    W = _weights(tr)
    p = tr._plan(M)
    _poison_all(tr, M)
    tr._eval_batch(M, X, idx, True)
    torch.cuda.synchronize()
    assert tr.read_state() == train0
    for t, t0 in zip((tr.params, tr.exp_avg, tr.exp_avg_sq, tr.w16, tr.w16t), arenas):
        assert ck.same_bits(t, t0)
    for t in [p["gpart"], tr.grads] + list(p["colsum"].values()) + [s for s, _ in p["slabs"].values()]:
        assert ck.untouched(t)
    rs = tr.read_state(eval=True)
    assert rs["step"] == step + 1 and rs["free_bits"] == 0.0
    b = _collect(tr, M, train=False, recon=True)
    b["ws_fwd"] = p["ws"]
    rows = Xc[idxc[cursor * B: cursor * B + M].long()]
    r = lk.check_forward(tr.spec, b, W, lk.plans(tr.spec, M), rows, tr.seed, EVAL_STREAM + tr.rng_stream, step, 0.0)
    assert f"F.{tr.spec[-1].name}.recon" in r and f"F.{tr.spec[-1].name}.dlog16" not in r
    bce, kld = b["bce_part"].double(), b["kld_part"].double()
    klw = rs["kl_beta"]
    bound = (bce.numel() + kld.numel() + lk.SLACK) * lk.U * (bce.abs().sum() + abs(klw) * kld.abs().sum())
    r["WG.loss"] = lk.ratio(torch.tensor(float(tr.loss_history(eval=True)[step]), dtype=torch.float64, device=dev),
                            bce.sum() + klw * kld.sum(), bound)
    _ok_all("eval.", r)


@pytest.mark.parametrize("image,z", [(28, 32), (128, 64)])
def test_decode_of_planted_latents_through_the_logits(image, z, native_ext):
    """``decode()`` on V = 1, 5 and B rows: z16 is the bf16 rounding of the planted latents, every decoder stage
    and the logits within their bounds, the result sigmoid(logits) bit for bit. V = B + 3 (two chunks) returns
    the rows of decode() on each chunk."""
    case = next(c for c in lk.CASES if c[1] == image and c[2] == z and c[5] == "spread")
    tr = _trainer(case)
    B, D, spec = tr.B, tr.D, tr.spec
    W = _weights(tr)
    zz = 1.5 * torch.randn(B + 3, z, generator=lk.gen(5)).cuda()
    outs = {}
    for V in (1, 5, B):
        for t, _ in _bufs(tr).values():
            _poison(t)
        out = tr.decode(zz[:V])
        torch.cuda.synchronize()
        outs[V] = out
        assert ck.same_bits(tr.z16.reshape(-1)[:V * z], zz[:V].to(torch.bfloat16).reshape(-1))
        assert ck.untouched(tr.logits, V * D) and ck.untouched(tr.xb) and ck.untouched(tr.mulv)
        acts = {}
        for l in tr.dec[:-1]:
            per = l.out_hw * l.out_hw * l.cout
            assert ck.untouched(tr.acts[l.name], V * per), l.name
            acts[l.name] = tr.acts[l.name][:V * per].reshape(-1, l.cout)
        b = dict(z16=tr.z16[:V], acts=acts, logits=tr.logits[:V * D])
        assert ck.same_bits(out.reshape(-1), torch.sigmoid(b["logits"]))
        r = lk.check_forward(spec, b, W, lk.plans(spec, V), None, 0, 0, 0, want=("dec",))
        assert f"F.{spec[-1].name}.logits" in r and len(r) == len(tr.dec)
        _ok_all(f"decode{V}.", r)
    tail = tr.decode(zz[B:])
    both = tr.decode(zz)
    assert ck.same_bits(both[:B], outs[B]) and ck.same_bits(both[B:], tail)


def test_zz_report_largest_ratios():
    """Not a check of its own: prints the largest error/bound ratio each output reached in this run."""
    for name in sorted(SEEN):
        print(f"MAXRATIO layer.{name} {SEEN[name]:.4g}")
    print(f"WALL module {time.time() - T0:.1f} s")
