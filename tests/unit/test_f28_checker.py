"""tests/f28_checker.py is not vacuous (CPU, no GPU): a plain torch f32
emulation of the whole fused 28x28 step -- every buffer the kernels store, bf16
stores at the kernels' rounding points -- passes every stage check at ratio
<= 1 on every case of the GPU test, each mutated emulation fails at the stage
its mutation belongs to and at no stage before it, and the input conditions of
the ``spread`` parameter set hold on every case."""
import math

import numpy as np
import pytest
import torch

from tests import f28_checker as fk
from tests import free_bits_cases as fbc
from tests import igemm_checker as ck

BF = torch.bfloat16
SEED, STREAM = 2, 0


# ---------------------------------------------------------------- emulation ----
def _bf(t, trunc=False):
    """The bf16 store of an f32 tensor: to nearest even, or (mutation) truncated."""
    if trunc:
        t = (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return t.to(BF)


def _conv(x, w):
    """f32 stride-2 4x4 conv, NHWC x [M, H, H, C], w [CO, 4, 4, C] -> [M OH OH, CO]."""
    return ck.im2col(x, 4, 2, 1) @ w.reshape(w.shape[0], -1).T


def _tconv(g, w, H):
    return ck.tconv_ref(g, w, 2, 1, H)


def emulate(P, X, idx, B, M, cursor, step, klw=1.0, fb=0.0, mut=None, recon=True):
    """One step in f32 -> (buffers, grads, slabs, loss). ``mut`` names one
    mutation (MUTATIONS)."""
    from multidisttorch_amd.ops.philox import reparam_eps

    W = fk.weights_of(P)
    f = {k: v.float() for k, v in W.items()}
    b = {}
    nob = lambda layer: 0.0 if mut == "nobias_" + layer else 1.0
    rows = X[idx[cursor * B: cursor * B + M].long()].float()
    b["xb"] = rows.clone()
    # ---- forward
    pre = _conv(rows.view(M, 28, 28, 1), f["W1f"]) + nob("enc1") * f["b1"]
    b["a1"] = _bf(torch.relu(pre)).view(M, 196, 32)
    cols = ck.im2col(b["a1"].float().view(M, 14, 14, 32), 4, 2, 1)
    if mut == "corner_tap":  # output pixel (6, 6) loses its tap (2, 2), input pixel (13, 13)
        cols = cols.clone().view(M, 49, 16, 32)
        cols[:, 48, 10, :] = 0
        cols = cols.view(M * 49, 512)
    pre = cols @ f["W2"].reshape(64, 512).T + nob("enc2") * f["b2"]
    b["a2"] = _bf(torch.relu(pre), trunc=mut == "trunc_store").view(M, fk.FLAT)
    b["mulv"] = b["a2"].float() @ f["Wh"].T + nob("enc_head") * f["bh"]
    mu, lv = b["mulv"][:, :32], b["mulv"][:, 32:]
    b["eps"] = torch.from_numpy(reparam_eps(M, 32, SEED, STREAM, step + (1 if mut == "philox_step" else 0)))
    sd = torch.exp(0.5 * lv)
    b["z16"] = _bf(mu + b["eps"] * sd)
    ksum = 1 + lv - mu * mu - sd * sd
    fl = (-0.5 * ksum < fb) if fb > 0 else torch.zeros_like(ksum, dtype=torch.bool)
    term = ksum if mut == "fb_fwd" else torch.where(fl, torch.full_like(ksum, -2 * fb), ksum)
    b["kld_part"] = -0.5 * term.sum(1)
    pre = b["z16"].float() @ f["Wd"].T + nob("dec_fc") * f["bd"]
    b["d0"] = _bf(torch.relu(pre))
    w3 = f["W3"].transpose(1, 2) if mut == "khkw_swap" else f["W3"]
    pre1 = _tconv(b["d0"].float().view(M, 7, 7, 64), w3, 14) + nob("dec1") * f["b3"]
    b["d1"] = _bf(torch.relu(pre1)).view(M, 196, 32)
    t = (_tconv(b["d1"].float().view(M, 14, 14, 32), f["W4f"], 28) + nob("dec2") * f["b4"]).view(M, 784)
    x = rows
    p = torch.sigmoid(t)
    if mut == "sat_trunc":  # the saturated branch cut short: p = 0 | 1 beyond |t| = 20
        p = torch.where(t < -20, torch.zeros_like(p), torch.where(t > 20, torch.ones_like(p), p))
    sp = torch.relu(t) + torch.log1p(torch.exp(-t.abs()))
    loss = x * torch.clamp(sp - t, max=100.0) + (1 - x) * torch.clamp(sp, max=100.0)
    b["dlog32"] = p - x
    if recon:
        b["recon"] = p
    b["bce_part"], b["db4_part"] = loss.sum(1), b["dlog32"].sum(1)
    # ---- backward
    mask1 = (torch.relu(pre1) > 0) if mut == "mask_pre" else (b["d1"].float().view(-1, 32) > 0)
    v = _conv(b["dlog32"].view(M, 28, 28, 1), f["W4f"]) * mask1
    b["gd1"] = _bf(v).view(M, 196, 32)
    vs = v.view(M, 196, 32)
    b["db3_part"] = (vs[:, :195] if mut == "pixel_missing" else vs).sum(1)
    v = _conv(b["gd1"].float().view(M, 14, 14, 32), f["W3"]) * (b["d0"].float().view(-1, 64) > 0)
    b["dbd_part"] = v.view(M, fk.FLAT)
    b["gd0"] = _bf(b["dbd_part"])
    dz = b["gd0"].float() @ f["Wd"]
    be = torch.where(torch.zeros_like(fl) if mut == "fb_bwd" else fl, torch.zeros_like(dz),
                     torch.full_like(dz, 1.0 if mut == "kl_weight" else klw))
    b["dmulv"] = torch.cat([dz + be * mu, 0.5 * dz * b["eps"] * sd + 0.5 * be * (sd * sd - 1)], 1)
    b["dmulv16"] = _bf(b["dmulv"])
    v = (b["dmulv"] @ f["Wh"]) * (b["a2"].float() > 0)
    b["ga2"] = _bf(v)
    vs = v.view(M, 49, 64)
    half1 = vs[:, 24:].sum(1)
    b["db2_part"] = torch.stack([vs[:, :24].sum(1), torch.zeros_like(half1) if mut == "db2_half" else half1])
    v = _tconv(b["ga2"].float().view(M, 7, 7, 64), f["W2"], 14) * (b["a1"].float().view(-1, 32) > 0)
    b["ga1"] = _bf(v).view(M, 196, 32)
    b["db1_part"] = v.view(M, 196, 32).sum(1)
    # ---- weight gradients and finalize
    grads, slabs = {}, {}
    for name, (H, C, CO, k, s, pd) in fk.WG_SHAPES.items():
        src = "dec1" if (mut == "wg_swap" and name == "enc2") else name
        inp = fk.wg_inputs(b, src)
        cols = ck.im2col(inp["X"].to(BF).float(), k, s, pd)
        g = (inp["G"].float().reshape(-1, CO).T @ cols).reshape(-1)
        rows_ = cols.shape[0]
        grads[name + ".weight"], slabs[name] = g, (g, 1, -(-rows_ // 64))
        key, per = fk.BIAS_SRCS[name]
        grads[name + ".bias"] = b[key].reshape(per * M, -1).sum(0)
    total = float(b["bce_part"].sum() + np.float32(klw) * b["kld_part"].sum())
    return b, grads, slabs, total


# mutation -> the stage that must be the first to fail
MUTATIONS = {
    "trunc_store": "P2", "corner_tap": "P2", "khkw_swap": "P6",
    "nobias_enc1": "P1", "nobias_enc2": "P2", "nobias_enc_head": "P3", "nobias_dec_fc": "P5", "nobias_dec1": "P6",
    "nobias_dec2": "P7",
    "mask_pre": "Q1", "pixel_missing": "Q1", "db2_half": "Q5", "kl_weight": "Q4", "fb_fwd": "P4", "fb_bwd": "Q4",
    "philox_step": "P4", "wg_swap": "WG", "sat_trunc": "P7",
}


# -------------------------------------------------------------------- inputs ----
@pytest.fixture(scope="module")
def base():
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=8, image=28, device=torch.device("cpu"), backend="torch", seed=SEED)
    init = {k: v.detach().clone() for k, v in tr.named_parameters().items()}
    return dict(init=init, spread=fk.spread_params(init), idx=fk.make_idx(),
                data={k: fk.make_data(k) for k in ("rand", "mnist", "bin")})


def _klw(step, knobs):
    if "kl_beta" in knobs:
        return float(np.float32(knobs["kl_beta"] * min(1.0, (step + 1) / knobs["kl_anneal_steps"])))
    return 1.0


def _run(base, case, mut=None, P=None):
    cid, B, M, pset, data, cursor, step, knobs = case
    P = base[pset] if P is None else P
    X, idx = base["data"][data], base["idx"]
    klw, fb = _klw(step, knobs), 0.0
    if knobs.get("free_bits"):
        b0 = emulate(P, X, idx, B, M, cursor, step, klw)[0]
        kl = fbc.kl_elements(b0["mulv"], 32)
        fb = float(np.float32(fbc.choose_floor(kl)))
        fbc.check_floor(kl, fb)
    b, grads, slabs, loss = emulate(P, X, idx, B, M, cursor, step, klw, fb, mut)
    rows = X[idx[cursor * B: cursor * B + M].long()]
    W = fk.weights_of(P)
    return b, W, fk.check_step(b, W, grads, slabs, loss, rows, SEED, STREAM, step, klw, fb)


# --------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("case", fk.CASES, ids=[c[0] for c in fk.CASES])
def test_emulation_passes_every_stage_and_meets_the_input_conditions(case, base):
    b, W, ratios = _run(base, case)
    bad = {k: r for k, r in ratios.items() if not r <= 1}
    assert not bad, bad
    assert set(fk.stage_of(k) for k in ratios) == set(fk.STAGES)
    cond = fk.input_conditions(b, W, case[3] == "spread", case[4] != "rand")
    assert all(cond.values()), cond


def test_cases_cover_what_the_gpu_test_needs():
    Ms = {c[2] for c in fk.CASES if c[1] == 128}
    assert {1, 2, 3, 77, 128} <= Ms
    assert {c[2] for c in fk.CASES if c[1] == 8} == {5, 8}
    live = [c for c in fk.CASES if c[5] != 0 and c[6] != 0]
    assert {3, 77} <= {c[2] for c in live}
    assert {c[4] for c in fk.CASES} == {"rand", "mnist", "bin"} and {c[3] for c in fk.CASES} == {"init", "spread"}
    kl = [c for c in fk.CASES if "kl_beta" in c[7]]
    assert kl and all(c[7]["kl_anneal_steps"] > c[6] + 1 and c[7]["kl_beta"] == 0.5 for c in kl)
    assert any(c[7].get("free_bits") for c in fk.CASES)
    for c in fk.CASES:
        assert c[5] < fk.NBATCH and fk.NBATCH * c[1] <= 512


def test_data_sets_are_what_they_claim():
    m, bn = fk.make_data("mnist"), fk.make_data("bin")
    img = m.view(-1, 28, 28)
    assert float(img[:, :4].abs().max()) == 0 and float(img[:, :, -4:].abs().max()) == 0
    assert bool((m == 1.0).any()) and bool(((m > 0) & (m < 1)).any())
    assert set(bn.unique().tolist()) == {0.0, 1.0}
    r = fk.make_data("rand")
    assert float(r.min()) >= 0 and float(r.max()) < 1


def test_spread_biases_are_all_nonzero(base):
    for k, v in base["spread"].items():
        if k.endswith(".bias"):
            assert bool((v != 0).all()), k


# the case the mutations run on: small, spread parameters, exact zeros in x, cursor and step live,
# a KL weight that is not 1 and a floor
MUT_CASE = ("mut", 128, 3, "spread", "mnist", 2, 5, {"kl_beta": 0.5, "kl_anneal_steps": 16, "free_bits": True})


def _underflow_params(P):
    """dec1 scaled so that its pre-activations are f32 subnormals around the
    smallest bf16 subnormal: a positive value below 2^-134 is stored as 0, and
    only then do the mask of the value before rounding and the mask of the
    stored activation differ."""
    Q = {k: v.clone() for k, v in P.items()}
    Q["dec1.weight"] = Q["dec1.weight"] * 1e-41
    Q["dec1.bias"] = Q["dec1.bias"] * 1e-41
    return Q


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_fails_at_its_own_stage(mut, base):
    P = _underflow_params(base["spread"]) if mut == "mask_pre" else None
    if P is not None:  # the planted case itself passes unmutated
        _, _, clean = _run(base, MUT_CASE, None, P)
        assert fk.first_failure(clean) is None, {k: r for k, r in clean.items() if not r <= 1}
    _, _, ratios = _run(base, MUT_CASE, mut, P)
    bad = {k: (r if math.isinf(r) else round(r, 3)) for k, r in ratios.items() if not r <= 1}
    assert fk.first_failure(ratios) == MUTATIONS[mut], (mut, bad)


def test_mutation_case_is_clean(base):
    _, _, ratios = _run(base, MUT_CASE)
    assert fk.first_failure(ratios) is None, {k: r for k, r in ratios.items() if not r <= 1}
