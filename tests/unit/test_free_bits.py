"""Free bits (``--free-bits``) off the GPU: the rule of both torch-backend
oracles against autograd on ``BCE + beta * sum max(fb, kl_d)``, the native CPU
step against the MLP oracle, the device-state plumbing on a host-resident
``TrialState``, spec / CLI parsing, checkpoints and the metrics of a run."""
import json
import math
import struct

import numpy as np
import pytest
import torch

from multidisttorch_amd.ckpt import checkpoint as ckpt
from multidisttorch_amd.data.datasets import synthetic_images
from multidisttorch_amd.hpo import runner
from multidisttorch_amd.hpo.runner import RunOptions, run_trial
from multidisttorch_amd.hpo.trial import TrialSpec, build_specs
from multidisttorch_amd.models.mlp_vae import arena_layout, init_params_, reference_step, views
from multidisttorch_amd.ops import native
from tests import free_bits_cases as fc

needs_native = pytest.mark.skipif(not native.available(), reason="native extension not built")
BETA = 4.0


# ------------------------------------------------------------------ the rule against autograd
def _mlp_case(M=24, D=36, H=20, Z=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    layout, numel, _ = arena_layout(D, H, Z)
    flat = torch.zeros(numel)
    init_params_(flat, layout, g)
    flat = flat.double()
    # spread mu / logvar so that kl_d covers a range (at init it is ~1e-3 everywhere)
    v = views(flat, layout)
    v["fc21.weight"].mul_(6.0)
    v["fc22.weight"].mul_(6.0)
    x = torch.rand(M, D, generator=g).double()
    eps = torch.randn(M, Z, generator=g).double()
    return layout, flat, x, eps, Z


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_mlp_oracle_matches_autograd_on_the_clamped_objective():
    layout, flat, x, eps, Z = _mlp_case()
    v = views(flat, layout)
    g0 = views(torch.zeros_like(flat), layout)
    f0 = reference_step(v, g0, x, eps, BETA)
    kl = fc.kl_elements(f0["mulv"], Z)
    fb = fc.choose_floor(kl)
    mask, share = fc.check_floor(kl, fb, margin=0.0)
    assert float((kl - fb).abs().min()) > 1e-6  # no element within 1e-6 of the floor
    gflat = torch.zeros_like(flat)
    f = reference_step(v, views(gflat, layout), x, eps, BETA, free_bits=fb)
    assert torch.equal(f["floored"], mask)
    # autograd on the objective written with torch.clamp
    p = flat.clone().requires_grad_()
    w = views(p, layout)
    h1 = torch.relu(x @ w["fc1.weight"].t() + w["fc1.bias"])
    mu = h1 @ w["fc21.weight"].t() + w["fc21.bias"]
    lv = h1 @ w["fc22.weight"].t() + w["fc22.bias"]
    z = mu + eps * torch.exp(0.5 * lv)
    t = torch.relu(z @ w["fc3.weight"].t() + w["fc3.bias"]) @ w["fc4.weight"].t() + w["fc4.bias"]
    bce = torch.nn.functional.binary_cross_entropy_with_logits(t, x, reduction="sum")
    loss = fc.objective(bce, mu, lv, BETA, fb)
    loss.backward()
    assert abs(float(f["loss"]) - float(loss.detach())) <= 1e-10 * abs(float(loss.detach()))
    for name, _, _ in layout:
        got, want = views(gflat, layout)[name], views(p.grad, layout)[name]
        assert _rel(got, want) < 1e-10, (name, _rel(got, want))
    # and the floor matters: without it the encoder gradients are other ones
    assert _rel(g0["fc21.weight"], views(p.grad, layout)["fc21.weight"]) > 1e-3


def test_mlp_oracle_without_a_floor_is_bitwise_the_plain_one():
    layout, flat, x, eps, Z = _mlp_case()
    v = views(flat.float(), layout)
    ga, gb = torch.zeros(flat.numel()), torch.zeros(flat.numel())
    fa = reference_step(v, views(ga, layout), x.float(), eps.float(), BETA)
    fb_ = reference_step(v, views(gb, layout), x.float(), eps.float(), BETA, free_bits=0.0)
    assert fa["floored"] is None and fb_["floored"] is None
    assert torch.equal(ga, gb) and torch.equal(fa["loss"], fb_["loss"])
    # today's formulas, spelled out
    mu, lv, sd = fa["mu"], fa["lv"], fa["sd"]
    assert torch.equal(fa["kld"], -0.5 * (1 + lv - mu * mu - sd * sd).sum())
    dz = fa["dh3"] @ v["fc3.weight"]
    assert torch.equal(fa["dmulv"][:, :Z], dz + BETA * mu)
    assert torch.equal(fa["dmulv"][:, Z:], 0.5 * dz * eps.float() * sd + 0.5 * BETA * (sd * sd - 1))


def _conv_model(seed=3):
    from multidisttorch_amd.models.conv_vae import TorchConvVAE, conv_vae_spec

    torch.manual_seed(seed)
    m = TorchConvVAE(conv_vae_spec(28, 1, 32), 28, 1, 32).double()
    with torch.no_grad():
        m.layers["enc_head"].weight.mul_(8.0)
    g = torch.Generator().manual_seed(seed)
    return m, torch.rand(6, 784, generator=g).double(), torch.randn(6, 32, generator=g).double()


def test_conv_oracle_matches_autograd_on_the_clamped_objective():
    m, x, eps = _conv_model()
    loss0, t, mu, lv = m.loss(x, eps, BETA)
    kl = fc.kl_elements(torch.cat([mu, lv], 1), 32)
    fb = fc.choose_floor(kl)
    fc.check_floor(kl, fb, margin=0.0)
    assert float((kl - fb).abs().min()) > 1e-6
    m.zero_grad(set_to_none=True)
    loss, *_ = m.loss(x, eps, BETA, fb)
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss0, t, mu, lv = m.loss(x, eps, BETA)
    bce = loss0 - BETA * (-0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp()))
    want_loss = fc.objective(bce, mu, lv, BETA, fb)
    want_loss.backward()
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-10 * abs(float(want_loss.detach()))
    for k, p in m.named_parameters():
        assert _rel(got[k], p.grad) < 1e-10, (k, _rel(got[k], p.grad))
    assert float(loss.detach()) > float(loss0.detach())  # floored elements add fb - kl_d > 0 each


def test_conv_oracle_without_a_floor_is_bitwise_the_plain_one():
    m, x, eps = _conv_model()
    m = m.float()
    x, eps = x.float(), eps.float()
    a, t, mu, lv = m.loss(x, eps, BETA)
    b, *_ = m.loss(x, eps, BETA, 0.0)
    assert torch.equal(a, b)
    xt = x.view(6, 28, 28, 1).permute(0, 3, 1, 2)
    sp = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    bce = (xt * torch.clamp(sp - t, max=100.0) + (1 - xt) * torch.clamp(sp, max=100.0)).sum()
    assert torch.equal(a, bce + BETA * (-0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp())))


def test_torch_trainers_take_the_floor():
    """Both trainers on the torch backend: the constructor argument reaches the
    step, read_state reports it (eval: 0), set_hparams changes and validates it."""
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    X = synthetic_images(64, seed=0)
    idx = torch.arange(64, dtype=torch.int32)
    for make in (lambda **kw: MlpVaeTrainer(batch_size=32, backend="torch", device="cpu", seed=1, kl_beta=BETA, **kw),
                 lambda **kw: ConvVaeTrainer(batch_size=32, backend="torch", device="cpu", seed=1, kl_beta=BETA, **kw)):
        a, b, c = make(), make(free_bits=0.0), make(free_bits=0.02)
        for tr in (a, b, c):
            tr.bind_train_data(X, idx)
            tr.set_cursor(0, 2)
            tr.train_steps(2)
        assert torch.equal(a.params, b.params) and (a.loss_history()[:2] == b.loss_history()[:2]).all()
        assert not torch.equal(a.params, c.params)
        assert c.loss_history()[0] > a.loss_history()[0]  # same weights and noise at step 0: only the floor differs
        assert c.read_state()["free_bits"] == float(np.float32(0.02)) and c.read_state(eval=True)["free_bits"] == 0.0
        assert a.read_state()["free_bits"] == 0.0
        c.set_hparams(free_bits=0.5)
        assert c.read_state()["free_bits"] == 0.5
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="free_bits"):
                c.set_hparams(free_bits=bad)
            with pytest.raises(ValueError, match="free_bits"):
                make(free_bits=bad)
        # evaluate reports the true ELBO terms whatever the floor
        c.load_state_dict(a.state_dict())
        assert a.evaluate(X, idx, want_first_recon=False)[0] == c.evaluate(X, idx, want_first_recon=False)[0]


# ------------------------------------------------------------------ native CPU step
@needs_native
@pytest.mark.parametrize("M", [32, 13])
def test_native_cpu_step_matches_the_oracle(M):
    """csrc/runtime/cpu_mlp.cpp against models/mlp_vae.py with 20-80 % of the
    elements floored, at the tolerances of tests/unit/test_cpu_mlp_step.py
    (loss rtol 1e-4; gradients rtol 1e-4 of the tensor's largest entry)."""
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
    from multidisttorch_amd.ops.philox import reparam_eps

    B, D, H, Z = 32, 64, 32, 8
    tr = MlpVaeTrainer(batch_size=B, D=D, H=H, Z=Z, backend="torch", device="cpu", seed=3, kl_beta=BETA)
    v = tr.named_parameters()
    with torch.no_grad():
        v["fc21.weight"].mul_(6.0)
        v["fc22.weight"].mul_(6.0)
    X = torch.rand(2 * B, D, generator=torch.Generator().manual_seed(3))
    idx = torch.randperm(2 * B, generator=torch.Generator().manual_seed(4)).to(torch.int32)
    x = X[idx[:M].long()]
    eps = torch.from_numpy(reparam_eps(M, Z, 3, 0, 0))
    v64 = {k: t.double() for k, t in v.items()}
    layout, numel, _ = arena_layout(D, H, Z)
    f0 = reference_step(v64, views(torch.zeros(numel, dtype=torch.float64), layout), x.double(), eps.double(), BETA)
    kl = fc.kl_elements(f0["mulv"], Z)
    fb = fc.choose_floor(kl)
    mask, share = fc.check_floor(kl, fb, lo=0.2, hi=0.8)
    gref = torch.zeros(numel, dtype=torch.float64)
    f = reference_step(v64, views(gref, layout), x.double(), eps.double(), BETA, free_bits=fb)
    assert torch.equal(f["floored"], mask)
    tr.set_hparams(free_bits=fb)
    cpu = tr._cpu_native()
    assert cpu is not None
    loss = cpu.forward_backward(tr._cpu_w, tr._cpu_g, X, idx, 0, M, 3, 0, 0, BETA, free_bits=fb)
    print(f"M={M}: {share:.2f} floored, loss {loss:.4f} vs {float(f['loss']):.4f}")
    np.testing.assert_allclose(loss, float(f["loss"]), rtol=1e-4)
    for name, got in tr.named_grads().items():
        ref = views(gref, layout)[name]
        torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))
    # the floor is seen: the same call without it gives other encoder gradients
    g_fb = tr.named_grads()["fc21.weight"].clone()
    cpu.forward_backward(tr._cpu_w, tr._cpu_g, X, idx, 0, M, 3, 0, 0, BETA)
    assert not torch.equal(tr.named_grads()["fc21.weight"], g_fb)
    with pytest.raises(ValueError, match="free_bits"):
        cpu.forward_backward(tr._cpu_w, tr._cpu_g, X, idx, 0, M, 3, 0, 0, BETA, free_bits=-1.0)


# ------------------------------------------------------------------ device state (host-resident)
FB_T, RING = 68, 72  # byte offsets in TrainState (csrc/kernels/vae_mlp.h): fb_t takes the former padding word


def _state(fb=None):
    s = native.require().TrialState(-1)
    kw = {} if fb is None else {"free_bits": fb}
    s.set_hparams(2e-3, 0.9, 0.999, 1e-8, 0.0, 2.0, 1.0, 3, False, **kw)
    return s


@needs_native
def test_state_layout_is_unchanged_and_fb_t_round_trips():
    C = native.require()
    s = _state(0.25)
    assert s.train_state.numel() == (RING + 4 * C.kLossHist + 63) // 64 * 64
    word = lambda t: struct.unpack("<f", bytes(t[FB_T:FB_T + 4].tolist()))[0]
    assert word(s.train_state) == 0.25 and word(s.eval_state) == 0.0
    assert s.read_state(False)[7] == 0.25 and s.read_state(True)[7] == 0.0
    # the neighbours keep their places: kl_t, kl_next, sched_off before it, the ring after it
    kl_t, kl_next, off = struct.unpack("<ffi", bytes(s.train_state[56:68].tolist()))
    assert (kl_t, kl_next, off) == (2.0, 2.0, 0)
    assert struct.unpack("<i", bytes(s.eval_state[64:68].tolist()))[0] == 1
    assert not s.loss_history(False).numpy().any()
    for ev in (False, True):
        s.set_step(ev, 7)  # re-seeds the effective values
        assert s.read_state(ev)[0] == 7 and s.read_state(ev)[7] == (0.0 if ev else 0.25)
    s.set_hparams(2e-3, 0.9, 0.999, 1e-8, 0.0, 2.0, 1.0, 3, False, free_bits=0.1)
    assert s.read_state(False)[7] == float(np.float32(0.1)) and s.read_state(True)[7] == 0.0
    assert s.read_state(False)[0] == 7
    # the default is no floor, and read_state keeps its first seven entries
    d = _state()
    assert d.read_state(False)[7] == 0.0 and len(d.read_state(False)) == 8
    assert d.read_state(False)[:7] == [0.0, 0.0, 0.0, 0.0, 0.0, 2e-3, 2.0]


@needs_native
@pytest.mark.parametrize("bad", [-0.01, float("nan"), float("inf")])
def test_state_refuses_bad_floors(bad):
    s = _state()
    with pytest.raises(ValueError, match="free_bits"):
        s.set_hparams(2e-3, 0.9, 0.999, 1e-8, 0.0, 2.0, 1.0, 3, False, free_bits=bad)
    assert s.read_state(False)[7] == 0.0


# ------------------------------------------------------------------ specs / CLI
def test_build_specs_free_bits():
    assert [s.free_bits for s in build_specs(3, 1)] == [0.0, 0.0, 0.0]
    assert [s.free_bits for s in build_specs(3, 1, free_bits=0.25)] == [0.25] * 3
    assert [s.free_bits for s in build_specs(3, 1, free_bits="0.5")] == [0.5] * 3
    assert [s.free_bits for s in build_specs(4, 1, free_bits="0,0.05")] == [0.0, 0.05, 0.0, 0.05]
    assert [s.free_bits for s in build_specs(2, 1, free_bits=[0.1, 0.2])] == [0.1, 0.2]
    assert TrialSpec(0, 1).free_bits == 0.0 and "free_bits" in TrialSpec(0, 1).to_dict()
    for bad in ("-0.1", "nan", "0.1,inf", "abc", -1.0, [0.1, float("nan")]):
        with pytest.raises(ValueError):
            build_specs(2, 1, free_bits=bad)


def _cli():
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    spec = importlib.util.spec_from_file_location("vae_hpo_cli", os.path.join(root, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag_parses_like_beta():
    cli = _cli()
    assert cli.parse_args([]).free_bits is None
    a = cli.parse_args(["--free-bits", "0,0.05", "--beta", "1,4"])
    assert a.free_bits == "0,0.05"
    specs = build_specs(2, 1, None, [1.0, 4.0], free_bits=a.free_bits)
    assert [(s.beta, s.free_bits) for s in specs] == [(1.0, 0.0), (4.0, 0.05)]


# ------------------------------------------------------------------ runner: checkpoints, metrics
B, N_TRAIN, N_TEST = 96, 320, 128


def _opts(model="mlp", **kw):
    return RunOptions(batch_size=B, backend="torch", results=False, synthetic=True, train_samples=N_TRAIN,
                      test_samples=N_TEST, model=model, quiet_train_log=True, **kw)


@pytest.fixture(scope="module")
def data():
    from multidisttorch_amd.data.datasets import ImageSet

    tr = synthetic_images(N_TRAIN, seed=0)
    te = synthetic_images(N_TEST, seed=1)
    return ImageSet(tr, (1, 28, 28), True, "synthetic28"), ImageSet(te, (1, 28, 28), True, "synthetic28")


def _spec(epochs, fb):
    return build_specs(1, epochs, None, None, 5, free_bits=fb)[0]


def test_checkpoint_records_the_floor_and_a_resume_checks_it(data, tmp_path, capsys):
    ck = str(tmp_path / "ck")
    res = run_trial(_spec(1, 0.05), None, _opts(ckpt_dir=ck), data=data)
    assert not res.failed, res.error
    raw = torch.load(ckpt.latest_path(ck, 0), weights_only=True)
    assert raw["objective"] == {"free_bits": 0.05} and raw["trial"]["free_bits"] == 0.05
    tr = runner._make_trainer(_spec(2, 0.05), _opts(), torch.device("cpu"), 0, 784, 8)
    assert ckpt.load_latest(ck, 0, tr)["free_bits"] == 0.05
    # the same floor resumes; another one (or none) is refused
    res = run_trial(_spec(2, 0.05), None, _opts(ckpt_dir=ck, resume=True), data=data)
    assert not res.failed and res.epochs == 1 and "resumed trial 0" in capsys.readouterr().out
    for other in (0.0, 0.1):
        with pytest.raises(ValueError, match="--free-bits 0.05"):
            run_trial(_spec(3, other), None, _opts(ckpt_dir=ck, resume=True), data=data)
    # a checkpoint from before the record was trained without a floor
    path = ckpt.latest_path(ck, 0)
    raw = torch.load(path, weights_only=True)
    del raw["objective"]
    torch.save(raw, path)
    assert ckpt.load_latest(ck, 0, tr)["free_bits"] == 0.0
    with pytest.raises(ValueError, match="--free-bits 0.0"):
        run_trial(_spec(3, 0.05), None, _opts(ckpt_dir=ck, resume=True), data=data)
    res = run_trial(_spec(3, 0.0), None, _opts(ckpt_dir=ck, resume=True), data=data)
    assert not res.failed and res.epochs == 1
    capsys.readouterr()


def test_metrics_carry_the_floor_only_when_asked(data, tmp_path, capsys):
    md = tmp_path / "m"
    run_trial(_spec(1, 0.0), None, _opts(metrics_dir=str(md)), data=data)
    rec = [json.loads(l) for l in open(md / "trial-0.jsonl")]
    assert rec and all("free_bits" not in r for r in rec)
    md2 = tmp_path / "m2"
    res = run_trial(_spec(1, 0.05), None,
                    _opts(metrics_dir=str(md2), report_objective=("free_bits",), latent_report=True), data=data)
    rec = [json.loads(l) for l in open(md2 / "trial-0.jsonl")]
    ep = [r for r in rec if "epoch" in r]
    assert ep and all(r["free_bits"] == float(np.float32(0.05)) for r in ep)
    lat = [r for r in rec if r.get("event") == "latent_eval"][0]
    assert lat["free_bits"] == 0.05
    assert lat["below_floor"] == sum(1 for v in lat["kl_per_dim"] if v < 0.05)
    assert res.extra["latent"]["below_floor"] == lat["below_floor"]
    # a trial without a floor in the same run reports its 0 and no below_floor
    md3 = tmp_path / "m3"
    run_trial(_spec(1, 0.0), None, _opts(metrics_dir=str(md3), report_objective=("free_bits",), latent_report=True),
              data=data)
    rec = [json.loads(l) for l in open(md3 / "trial-0.jsonl")]
    assert all(r["free_bits"] == 0.0 for r in rec if "epoch" in r)
    assert "below_floor" not in [r for r in rec if r.get("event") == "latent_eval"][0]
    capsys.readouterr()
    assert math.isfinite(res.final_test_loss)
