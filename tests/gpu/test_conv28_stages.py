"""The fused 28x28 conv-VAE step (csrc/kernels/conv28_fused.h, conv28_pair.h,
conv28_fused.hip) per element and stage by stage on one MI355X, against the
chained float64 oracles and derived bounds of tests/f28_checker.py (``fk``),
which tests/unit/test_f28_checker.py shows to be non-vacuous.

Every case of ``fk.CASES`` (batches M = 1, 2, 3, 77, 128 of B = 128 and M = 5, 8
of B = 8 -- the trainer accepts a smaller B --, the initial and the ``spread``
parameters, uniform / MNIST-like / binarized rows, cursor and step != 0, a KL
weight on its anneal ramp, a free-bits floor) runs one step on each of the four
forms: two launches, merged solo, paired, and paired with every partner late
(the solo fallback). Before the step every output buffer is poisoned over its
whole allocation (NaN, or BF16_FILL for bf16); after it every stage is checked
against the oracle, rows >= M of every per-sample buffer must still hold the
poison, and ``f28_err`` must be 0. One more test per form checks the step that
follows another, whose rows the previous finalize gathered. The eval tests check ``recon`` of a forward
launch that stores the chain, and the trainer's eval pass (solo and paired)
bit for bit against it. Each check prints ``RATIO f28.<stage>.<output>
<error/bound>``; the last test prints the largest ratio per output."""

import numpy as np
import pytest
import torch

from tests import f28_checker as fk
from tests import free_bits_cases as fbc
from tests import igemm_checker as ck

pytestmark = pytest.mark.gpu

SEED = 2
SEEN = {}
FORMS = {"two-launch": dict(merge=False, pair=False, delay=0), "merged": dict(merge=True, pair=False, delay=0),
         "paired": dict(merge=True, pair=True, delay=0), "paired-late": dict(merge=True, pair=True, delay=30)}
_DATA = {}


def _ok(name, r):
    SEEN[name] = max(SEEN.get(name, 0.0), r)
    print(f"RATIO f28.{name} {r:.4g}")
    assert r <= 1, (name, r)


def _data(kind, dev):
    if kind not in _DATA:
        _DATA[kind] = fk.make_data(kind)
    if "idx" not in _DATA:
        _DATA["idx"] = fk.make_idx()
    return _DATA[kind], _DATA["idx"], _DATA[kind].to(dev), _DATA["idx"].to(dev)


def _trainer(B, pset, knobs, fb=0.0):
    from multidisttorch_amd.hpo.schedule import Schedule
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    kw = {}
    if "kl_beta" in knobs:
        kw = dict(kl_beta=knobs["kl_beta"], schedule=Schedule(kl_anneal_steps=knobs["kl_anneal_steps"]))
    tr = ConvVaeTrainer(batch_size=B, image=28, device=torch.device("cuda"), backend="hip", seed=SEED,
                        use_graphs=False, free_bits=fb, **kw)
    assert tr.f28
    if pset == "spread":
        init = {k: v.detach().cpu().clone() for k, v in tr.named_parameters().items()}
        with torch.no_grad():
            for k, v in fk.spread_params(init).items():
                tr.named_parameters()[k].copy_(v)
        tr.refresh_weights()
    tr.f28_skip_adam = True
    return tr


def _buffers(tr):
    """name -> (tensor over the whole allocation, elements per sample) of every per-sample output of the step."""
    B = tr.B
    bce, kld, db4 = tr._parts28()
    bias = tr.f28_bias
    t = {"xb": tr.xb, "a1": tr.acts["enc1"], "a2": tr.acts["enc2"], "mulv": tr.mulv, "eps": tr.eps, "z16": tr.z16,
         "d0": tr.acts["dec_fc"], "d1": tr.acts["dec1"], "dlog32": tr.dlog32, "bce_part": bce, "kld_part": kld,
         "db4_part": db4, "gd1": tr.gacts["dec1"], "gd0": tr.gacts["dec_fc"], "ga2": tr.gacts["enc2"],
         "ga1": tr.gacts["enc1"], "dmulv": tr.dmulv, "dmulv16": tr.dmulv16,
         "dbd_part": bias.narrow(0, 0, B * 3136), "db3_part": bias.narrow(0, B * 3136, B * 32),
         "db2_part": bias.narrow(0, B * 3168, 2 * B * 64), "db1_part": bias.narrow(0, B * 3296, B * 32)}
    for k, v in t.items():
        assert v.numel() == B * fk.BUFS[k][0] and (v.dtype == torch.float32) == (fk.BUFS[k][1] == "f"), k
    return t


def _poison(t):
    t.fill_(float("nan") if t.dtype == torch.float32 else fk.BF16_FILL)


def _collect(bufs, M, keys):
    """The first M rows of each buffer on the CPU, and that every later row still holds the poison."""
    out = {}
    for k in keys:
        t, per = bufs[k].reshape(-1), fk.BUFS[k][0]
        assert ck.untouched(t, M * per), f"{k}: rows >= {M} were written"
        v = t[:M * per].cpu()
        out[k] = v.reshape(2, M, 64) if k == "db2_part" else v.reshape((M,) + fk.SHAPES.get(k, (per,)))
    return out


FWD_KEYS = ("xb", "a1", "a2", "mulv", "eps", "z16", "d0", "d1", "dlog32", "bce_part", "kld_part", "db4_part")


def _conditions(b, W, case):
    cond = fk.input_conditions(b, W, case[3] == "spread", case[4] != "rand")
    assert all(cond.values()), cond


def _one_step(case, form, fb=0.0, warm=False):
    """One step of the case on the form -> (trainer, stored buffers, weights, ratios). ``warm``: a step runs
    first, so the checked one (step + 1, cursor + 1) takes its rows from the previous finalize's gather."""
    from multidisttorch_amd.ops.conv_plans import wgrad_plan

    cid, B, M, pset, data, cursor, step, knobs = case
    dev = torch.device("cuda")
    Xc, idxc, X, idx = _data(data, dev)
    tr = _trainer(B, pset, knobs, fb)
    f = FORMS[form]
    tr.f28_merge, tr.f28_pair, tr.f28_pair_delay_us = f["merge"], f["pair"], f["delay"]
    if f["pair"]:  # slot 15 of a workgroup's stamps: the mode it ran in (obs/f28_phases.py)
        tr.f28_stamps = tuple(torch.zeros(2 * B * 16, dtype=torch.int64, device=dev) for _ in range(2))
    tr.bind_train_data(X, idx)
    tr.set_step(step)
    tr.set_cursor(cursor, fk.NBATCH)
    W = fk.weights_from_list(tr._f28_weights())
    plan = tr._plan28(M)
    if warm:
        tr.train_steps(1, M=M)
        step, cursor = step + 1, (cursor + 1) % fk.NBATCH
        assert tr.f28_prefetch and bool((tr.f28_xtag[:M] == step).all())  # P0's one-round-trip path
    bufs = _buffers(tr)
    for t in bufs.values():
        _poison(t)
    _poison(tr.grads)
    for name in fk.WG_SHAPES:
        _poison(plan["slabs"][name + ".weight"][0])
    p0 = tr.params.clone()
    tr.train_steps(1, M=M)
    torch.cuda.synchronize()
    assert int(tr.f28_err.item()) == 0 and int(tr.f28_pairw.abs().sum()) == 0
    assert torch.equal(tr.params, p0)
    if f["pair"]:
        # modes: 0 solo, 1 | 2 the two halves of a pair, 3 a partner that found its sample taken. Pairing never
        # assumes co-residency, so only the late form's outcome is fixed: every leader solo, every partner out
        modes = (tr.f28_stamps[0].view(2 * B, 16)[:2 * M, 15] & 15).cpu()
        n = [int((modes == m).sum()) for m in range(4)]
        print(f"workgroup modes of {form}: solo {n[0]}, role 0 {n[1]}, role 1 {n[2]}, out {n[3]}")
        assert n[1] == n[2] and n[0] == n[3] and n[0] + n[1] == M, n
        if f["delay"]:
            assert n[0] == M and bool((modes[:M] == 0).all()), n
    st = tr.read_state()
    assert st["step"] == step + 1 and st["cursor"] == (cursor + 1) % fk.NBATCH
    klw, fbk = st["kl_beta"], st["free_bits"]
    if "kl_beta" in knobs:
        want = float(np.float32(knobs["kl_beta"] * (step + 1) / knobs["kl_anneal_steps"]))
        assert klw == want and 0 < klw < knobs["kl_beta"], (klw, want)
    else:
        assert klw == 1.0
    assert fbk == float(np.float32(fb))
    b = _collect(bufs, M, fk.BUFS)
    grads = {k: v.detach().cpu().clone() for k, v in tr.named_grads().items()}
    slabs = {}
    for name in fk.WG_SHAPES:
        t, ns = plan["slabs"][name + ".weight"]
        wp = wgrad_plan(tr._desc(tr.by_name[name], M))
        assert wp.nsplit == ns
        slabs[name] = (t.cpu(), ns, wp.mt_per_split)
    loss = float(tr.loss_history()[step])
    rows = Xc[idxc[cursor * B: cursor * B + M].long()]
    ratios = fk.check_step(b, W, grads, slabs, loss, rows, tr.seed, tr.rng_stream, step, klw, fbk)
    return tr, b, W, ratios


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", fk.CASES, ids=[c[0] for c in fk.CASES])
def test_every_stage_of_the_step_within_its_bound(case, form, native_ext):
    fb = 0.0
    if case[7].get("free_bits"):
        # the floor comes from the step without one: the midpoint of the widest gap of its kl_d values, with
        # every element away from it, so the kernels must floor exactly the float64 set
        _, b0, _, _ = _one_step(case, form)
        kl = fbc.kl_elements(b0["mulv"], 32)
        fb = float(np.float32(fbc.choose_floor(kl)))
        mask, share = fbc.check_floor(kl, fb)
        print(f"floor {fb:.6g}: {share:.3f} of the elements floored")
    tr, b, W, ratios = _one_step(case, form, fb)
    _conditions(b, W, case)
    if fb:
        assert torch.equal(fk.floored_set(b["mulv"], fb), mask)
    assert set(fk.stage_of(k) for k in ratios) == set(fk.STAGES)
    bad = {}
    for k, r in ratios.items():
        try:
            _ok(k, r)
        except AssertionError:
            bad[k] = r
    assert not bad, bad


@pytest.mark.parametrize("form", list(FORMS))
def test_step_on_prefetched_rows_within_its_bounds(form, native_ext):
    """The step as training runs it: its batch rows were gathered by the previous step's finalize (f28_xn,
    tagged with the step they are for), so P0 takes them without the cursor -> index -> row chain."""
    case = next(c for c in fk.CASES if c[0] == "m77-spread-mnist")
    tr, b, W, ratios = _one_step(case, form, warm=True)
    _conditions(b, W, case)
    for k, r in ratios.items():
        _ok("prefetched." + k, r)


@pytest.mark.parametrize("M", [3, 77])
def test_eval_forward_recon_and_eval_pass_bitwise(M, native_ext):
    """``f28_forward`` with train = True and a recon tensor stores the chain:
    every forward stage and recon against the oracle. The trainer's eval pass
    (train = False), solo and paired, then gives recon, bce_part and kld_part
    bit for bit on the same rows, eval state and stream."""
    from multidisttorch_amd.models.trainer_base import EVAL_STREAM

    case = next(c for c in fk.CASES if c[0] == "m77-spread-mnist")
    B, cursor, step = case[1], 1, 3
    dev = torch.device("cuda")
    Xc, idxc, X, idx = _data(case[4], dev)
    tr = _trainer(B, case[3], {})
    tr.f28_pair = True
    st = tr.state

    def reset():
        tr.set_cursor(cursor, fk.NBATCH, eval=True)
        st.set_step(True, step)

    reset()
    assert tr.read_state(eval=True)["free_bits"] == 0.0
    bufs = _buffers(tr)
    bufs["recon"] = tr.recon
    for t in bufs.values():
        _poison(t)
    table = tr._fwd_table28(X, idx, st.eval_state, True, recon=tr.recon)
    stream = EVAL_STREAM + tr.rng_stream
    tr.C.f28_forward(table, B, M, stream, True)
    torch.cuda.synchronize()
    W = fk.weights_from_list(tr._f28_weights())
    b = _collect(bufs, M, FWD_KEYS)
    assert ck.untouched(tr.recon.reshape(-1), M * 784)
    b["recon"] = tr.recon[:M * 784].cpu().reshape(M, 784)
    _conditions(b, W, case)
    rows = Xc[idxc[cursor * B: cursor * B + M].long()]
    ratios = fk.check_forward(b, W, rows, tr.seed, stream, step, 0.0)
    assert "P7.recon" in ratios
    for k, r in ratios.items():
        _ok("eval." + k, r)
    want = {k: bufs[k].reshape(-1)[:M * fk.BUFS.get(k, (784,))[0]].clone() for k in ("recon", "bce_part", "kld_part")}
    assert tr.read_state(eval=True)["step"] == step  # the bare launch advances nothing
    for pair in (False, True):
        for k in want:
            _poison(bufs[k])
        reset()
        tr._eval_pair = pair
        tr._eval_batch28(M, X, idx, True)
        torch.cuda.synchronize()
        assert int(tr.f28_err.item()) == 0 and int(tr.f28_pairw.abs().sum()) == 0
        assert tr.read_state(eval=True)["step"] == step + 1
        for k, w in want.items():
            got = bufs[k].reshape(-1)
            assert ck.same_bits(got[:w.numel()], w), (k, pair)
            assert ck.untouched(got, w.numel()), (k, pair)


def test_zz_report_largest_ratios():
    """Not a check of its own: prints the largest error/bound ratio each output reached in this run."""
    for name in sorted(SEEN):
        print(f"MAXRATIO f28.{name} {SEEN[name]:.4g}")
