"""The checker of the conv-VAE small-kernel tests (tests/conv_small_checker.py)
is not vacuous. For every oracle: (a) it agrees with an independent float64
route; (b) a plain f32 torch emulation of the kernel's formula passes the
bound at the GPU test's inputs, and each mutated emulation (a bug the suite
could not see before) fails it on at least one element. Mutants live in these
emulations only; no mutated kernel exists."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multidisttorch_amd.models.mlp_vae import reference_adam_
from multidisttorch_amd.ops.philox import reparam_eps
from tests import conv_small_checker as ck

F32 = torch.float32
SHAPES = [(5, 8), (37, 24)]   # the GPU test's reparam shapes


def _eps(B, Z, seed=0, stream=0, step=0):
    return torch.from_numpy(reparam_eps(B, Z, seed, stream, step))


# ------------------------------------------------------- f32 emulations ----
def emu_reparam(mulv, eps, mut=None):
    Z = mulv.shape[1] // 2
    mu, lv = mulv[:, :Z], mulv[:, Z:]
    if mut == "swap_halves":
        mu, lv = lv, mu
    sd = torch.exp(0.5 * lv)
    return mu + eps * sd, -0.5 * (1 + lv - mu * mu - sd * sd)


def emu_reparam_bwd(g, mulv, eps, beta, mut=None):
    Z = mulv.shape[1] // 2
    mu, lv = mulv[:, :Z], mulv[:, Z:]
    if mut == "swap_halves":
        mu, lv = lv, mu
    beta = torch.tensor(beta, dtype=F32)
    sd = torch.exp(0.5 * lv)
    if mut == "beta_on_dz":
        dm, dl = beta * g + mu, 0.5 * beta * g * eps * sd + 0.5 * (sd * sd - 1)
    elif mut == "no_minus_one":
        dm, dl = g + beta * mu, 0.5 * g * eps * sd + 0.5 * beta * (sd * sd)
    else:
        dm, dl = g + beta * mu, 0.5 * g * eps * sd + 0.5 * beta * (sd * sd - 1)
    return torch.cat([dm, dl], 1)


def emu_slab_sum(slab, ks, bias=None, mut=None):
    s = torch.zeros_like(slab[0])
    for z in range(ks - 1 if mut == "drop_last" else ks):
        s = s + slab[z]
    return s if bias is None else s + bias


def emu_bce(t, x, mut=None):
    sp = torch.log1p(torch.exp(t)) if mut == "no_split" else torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    cap = math.inf if mut == "no_clamp" else 100.0
    loss = x * torch.clamp(sp - t, max=cap) + (1 - x) * torch.clamp(sp, max=cap)
    p = 1 / (1 + torch.exp(-t))
    return loss, p, p - x


def emu_adam(p, g, m, v, c, mut=None):
    """adam_update of adam_common.h in f32 (constants rounded as AdamC holds them)."""
    k = {n: torch.tensor(c[n], dtype=F32) for n in ("step_size", "bc2s", "b1", "b2", "eps", "wd", "gs", "lr", "omb1",
                                                    "omb2")}
    decoupled = c["decoupled"]
    if mut == "swap_decay":
        decoupled = not decoupled
    if mut == "torch_omb2":   # float32(1 - beta2) of the double beta2, torch's weight
        k["omb2"] = torch.tensor(1.0 - 0.999, dtype=F32)
    gr = g if mut == "no_grad_scale" else g * k["gs"]
    if c["wd"] != 0:
        if decoupled:
            p = p * (1 - k["lr"] * k["wd"])
        else:
            gr = k["wd"] * p + gr
    m = m + k["omb1"] * (gr - m)
    v = k["omb2"] * (gr * gr) + v * k["b2"]
    den = v.sqrt() / k["bc2s"] + k["eps"]
    return p - k["step_size"] * (m / den), m, v


# ------------------------------------------------ (a) independent routes ----
@pytest.mark.parametrize("B,Z", SHAPES)
@pytest.mark.parametrize("beta", [1.0, 0.5, 0.2])
def test_reparam_bwd_ref_is_the_autograd_gradient(B, Z, beta):
    mulv = ck.reparam_inputs(B, Z).double().requires_grad_()
    eps = _eps(B, Z).double()
    g = torch.randn(B, Z, generator=ck.gen(1), dtype=torch.float64)
    z, _, bk, _, _ = ck.reparam_ref(mulv, eps, beta)
    (want,) = torch.autograd.grad((g * z).sum() + bk.sum(), mulv)
    got, _ = ck.reparam_bwd_ref(g, mulv.detach(), eps, beta)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_reparam_ref_kld_is_the_closed_form():
    mulv = ck.reparam_inputs(37, 24).double()
    mu, lv = mulv[:, :24], mulv[:, 24:]
    q = torch.distributions.Normal(mu, torch.exp(0.5 * lv))
    want = torch.distributions.kl_divergence(q, torch.distributions.Normal(0.0, 1.0))
    _, k, _, _, _ = ck.reparam_ref(mulv, torch.zeros(37, 24))
    torch.testing.assert_close(k, want.double(), rtol=1e-10, atol=1e-12)


def test_bce_ref_matches_torch_bce():
    t, x = ck.bce_inputs(3, 100)
    assert float(t.abs().max()) == 120.0
    r = ck.bce_ref(t, x)
    t, x = t.double(), x.double()
    one = torch.ones_like(t)
    # torch's BCE (log clamped at -100) per target class: BCE(sigmoid(t), x) is linear in x, and its
    # x = 0 part is BCE(sigmoid(-t), 1), which unlike log(1 - sigmoid(t)) keeps its precision for t > 37
    want = (x * F.binary_cross_entropy(torch.sigmoid(t), one, reduction="none")
            + (1 - x) * F.binary_cross_entropy(torch.sigmoid(-t), one, reduction="none"))
    torch.testing.assert_close(r["loss"], want, rtol=1e-10, atol=1e-15)   # sigmoid(t) itself is within 1e-16
    near = t.abs() <= 15   # ... and directly, where 1 - sigmoid(t) is still accurate
    direct = F.binary_cross_entropy(torch.sigmoid(t), x, reduction="none")
    torch.testing.assert_close(r["loss"][near], direct[near], rtol=1e-8, atol=1e-12)
    # the clamp bites at +-120 (and only there among the planted logits)
    assert float(r["loss"].max()) == 100.0 and int((r["loss"] == 100.0).sum()) == 4
    torch.testing.assert_close(r["g"], torch.sigmoid(t) - x, rtol=0, atol=0)


@pytest.mark.parametrize("name", list(ck.ADAM_SETS))
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_ref_matches_torch_optim(name, step):
    hp = ck.ADAM_SETS[name]
    p0, g, m0, v0 = (t.double() for t in ck.adam_inputs(1028))
    b1, b2 = hp["beta1"], hp["beta2"]
    c = ck.adam_consts(hp, step, omb=(1 - b1, 1 - b2))
    c.update(b1=b1, b2=b2, eps=hp["eps"], wd=hp["weight_decay"], gs=hp["grad_scale"])   # torch's double scalars
    got = ck.adam_ref(p0, g, m0, v0, c)[:3]
    # route 1: the project's flat-tensor reference
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    reference_adam_(p, g, m, v, step, c["lr"], b1, b2, hp["eps"], hp["weight_decay"], hp["grad_scale"], hp["decoupled"])
    for a, b in zip(got, (p, m, v)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-14)
    # route 2: torch.optim at the same state (grad_scale applied to the gradient beforehand)
    w = torch.nn.Parameter(p0.clone())
    cls = torch.optim.AdamW if hp["decoupled"] else torch.optim.Adam
    opt = cls([w], lr=c["lr"], betas=(b1, b2), eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False)
    opt.state[w] = dict(step=torch.tensor(float(step - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    w.grad = g * hp["grad_scale"]
    opt.step()
    st = opt.state[w]
    for a, b in zip(got, (w.detach(), st["exp_avg"], st["exp_avg_sq"])):
        torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-14)


def test_slab_sum_ref_is_the_fsum():
    slab, bias = ck.slab_inputs(33, 3, 8, True)
    ref, bound = ck.slab_sum_ref(slab[:33], bias)
    want = [[math.fsum([float(v) for v in slab[:33, i, j]] + [float(bias[j])]) for j in range(16)] for i in range(3)]
    torch.testing.assert_close(ref, torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=1e-15)
    assert bool((bound > 0).all())


# ------------------------------------------- (b) emulations and mutants ----
@pytest.mark.parametrize("B,Z", SHAPES)
def test_reparam_emulation_passes_and_mutants_fail(B, Z):
    mulv, eps = ck.reparam_inputs(B, Z), _eps(B, Z)
    z, k, _, bz, bk = ck.reparam_ref(mulv, eps)
    own = ck.block_owners(B, Z)
    kref, kb = ck.block_sum_ref(k, bk, own)

    def ratios(mut):
        gz, gk = emu_reparam(mulv, eps, mut)
        part = torch.stack([gk.reshape(-1)[o].sum() for o in own])
        return ck.ratio(gz, z, bz), ck.ratio(gk, k, bk), ck.ratio(part, kref, kb)

    assert max(ratios(None)) <= 1, ratios(None)
    assert min(ratios("swap_halves")) > 1, ratios("swap_halves")


def test_noise_key_is_the_step_before_the_state():
    B, Z, seed, stream, step = 5, 8, 2 ** 32 + 7, 3, 2 ** 32 + 5
    assert ck.eps_ratio(_eps(B, Z, seed, stream, step - 1), B, Z, seed, stream, step) == 0.0
    mutants = dict(step_t=_eps(B, Z, seed, stream, step), no_step_hi=_eps(B, Z, seed, stream, (step - 1) & 0xFFFFFFFF),
                   no_seed_hi=_eps(B, Z, seed & 0xFFFFFFFF, stream, step - 1), no_stream=_eps(B, Z, seed, 0, step - 1))
    for name, e in mutants.items():
        assert ck.eps_ratio(e, B, Z, seed, stream, step) > 1, name


@pytest.mark.parametrize("B,Z", SHAPES)
@pytest.mark.parametrize("beta", [0.5, ck.f32(0.5 * 0.4)])
def test_reparam_bwd_emulation_passes_and_mutants_fail(B, Z, beta):
    mulv, eps = ck.reparam_inputs(B, Z), _eps(B, Z)
    g = torch.randn(B, Z, generator=ck.gen(2))
    ref, bound = ck.reparam_bwd_ref(g, mulv, eps, beta)
    assert ck.ratio(emu_reparam_bwd(g, mulv, eps, beta), ref, bound) <= 1
    for mut in ("no_minus_one", "beta_on_dz", "swap_halves"):
        assert ck.ratio(emu_reparam_bwd(g, mulv, eps, beta, mut), ref, bound) > 1, mut


@pytest.mark.parametrize("Z,fwd", [(8, True), (8, False), (256, True), (24, True), (40, False)])
def test_slab_sum_emulation_passes_and_dropped_slice_fails(Z, fwd):
    grid = ck.row_ks(Z, fwd) if ck.rows_ok(Z) else ck.ELEM_KS
    for ks in grid:
        slab, bias = ck.slab_inputs(ks, 3, Z, fwd)
        for b in (None, bias) if fwd else (None,):
            ref, bound = ck.slab_sum_ref(slab[:ks], b)
            assert ck.ratio(emu_slab_sum(slab, ks, b), ref, bound) <= 1, ks
            assert ck.ratio(emu_slab_sum(slab, ks, b, "drop_last"), ref, bound) > 1, ks
            assert ck.ratio(emu_slab_sum(slab, ks + 1, b), ref, bound) == math.inf   # the NaN slice beyond ks


def test_combine_bound_carries_the_slab_bound():
    """dz with an error of its full slab bound still passes the dmulv check
    fed that bound (and fails without it)."""
    B, Z, ks = 3, 32, 33
    slab, _ = ck.slab_inputs(ks, B, Z, False)
    dz, bz = ck.slab_sum_ref(slab[:ks])
    mulv, eps = ck.reparam_inputs(B, Z), _eps(B, Z)
    ref, bound = ck.reparam_bwd_ref(dz, mulv, eps, 0.5, bz)
    off, _ = ck.reparam_bwd_ref(dz + 0.9 * bz, mulv, eps, 0.5)
    assert ck.ratio(off, ref, bound) <= 1
    assert ck.ratio(off, ref, ck.reparam_bwd_ref(dz, mulv, eps, 0.5)[1]) > 1


@pytest.mark.parametrize("B,P", [(3, 100), (2, 784)])
def test_bce_emulation_passes_and_mutants_fail(B, P):
    t, x = ck.bce_inputs(B, P)
    r = ck.bce_ref(t, x)
    own = ck.block_owners(1, B * P)

    def ratios(mut):
        loss, p, g = emu_bce(t, x, mut)
        part = torch.stack([loss.reshape(-1)[o].sum() for o in own])
        gpart = torch.stack([g.reshape(-1)[o].sum() for o in own])
        pr, pb = ck.block_sum_ref(r["loss"], r["b_loss"], own)
        gr, gb = ck.block_sum_ref(r["g"], r["b_g"], own)
        d16 = g.to(torch.bfloat16)
        return dict(loss=ck.ratio(loss, r["loss"], r["b_loss"]), p=ck.ratio(p, r["p"], r["b_p"]),
                    g=ck.ratio(g, r["g"], r["b_g"]), part=ck.ratio(part, pr, pb), gpart=ck.ratio(gpart, gr, gb),
                    dlog16=ck.ratio(d16, r["g"], ck.bf16_bound(r["g"], r["b_g"])))

    ok = ratios(None)
    assert max(ok.values()) <= 1, ok
    for mut in ("no_clamp", "no_split"):   # the planted +-120 (clamp) and +95 (log1p(exp(95)) = inf) logits
        bad = ratios(mut)
        assert bad["loss"] > 1 and bad["part"] > 1, (mut, bad)
    # a bf16 store that truncates instead of rounding to nearest leaves the dlog16 bound
    g = emu_bce(t, x)[2]
    trunc = (g.view(torch.int32) & -65536).view(F32)
    assert ck.ratio(trunc, r["g"], ck.bf16_bound(r["g"], r["b_g"])) > 1


@pytest.mark.parametrize("name", list(ck.ADAM_SETS))
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_emulation_passes_and_mutants_fail(name, step):
    hp = ck.ADAM_SETS[name]
    p, g, m, v = ck.adam_inputs(1028)
    assert int(((g * hp["grad_scale"]) ** 2 > 77).sum()) > 50
    c = ck.adam_consts(hp, step)
    rp, rm, rv, bp, bm, bv = ck.adam_ref(p, g, m, v, c)

    def ratios(mut):
        gp, gm, gv = emu_adam(p, g, m, v, c, mut)
        return ck.ratio(gp, rp, bp), ck.ratio(gm, rm, bm), ck.ratio(gv, rv, bv)

    assert max(ratios(None)) <= 1, ratios(None)
    assert ratios("torch_omb2")[2] > 1            # exp_avg_sq sees the other 1 - beta2 once g^2 > 77
    if hp["grad_scale"] != 1.0:
        assert min(ratios("no_grad_scale")) > 1
    if hp["weight_decay"] != 0:                   # coupled applied as decoupled, and the reverse
        assert ratios("swap_decay")[1] > 1        # exp_avg gains / loses the wd * p term


def test_adam_consts_follow_the_f32_moment_weight_convention():
    c = ck.adam_consts(ck.ADAM_SETS["default"], 1)
    assert c["omb2"] == float(np.float32(1) - np.float32(0.999)) != float(np.float32(1 - 0.999))
    assert abs(c["omb2"] / float(np.float32(1 - 0.999)) - 1) > 1e-5   # the 1.3e-5 of adam_common.h
    w = ck.adam_consts(ck.ADAM_SETS["decoupled"], 1000)
    assert w["lr"] == 2e-3 * 0.25 and not ck.adam_consts(ck.ADAM_SETS["decoupled"], 1)["lr"] == 2e-3


def test_block_owners_cover_every_element_once():
    for B, Z, ks in [(5, 8, None), (37, 24, None), (3, 8, 7), (3, 256, 40), (3, 512, 17), (3, 24, 300), (3, 40, 1)]:
        own = ck.block_owners(B, Z, ks)
        assert torch.equal(torch.cat(own), torch.arange(B * Z))
        if ks is not None and ck.rows_ok(Z):
            assert len(own) == B
    assert not ck.rows_ok(512) and ck.rows_ok(256) and not ck.rows_ok(24) and not ck.rows_ok(4)
    assert [ck.splitk_rp(k) for k in ck.ELEM_KS] == [1, 2, 8, 64]
    assert ck.row_ks(32, True) == [1, 3, 16, 256, 257, 533] and ck.row_ks(512, True) == [1, 3, 16, 17, 38]
