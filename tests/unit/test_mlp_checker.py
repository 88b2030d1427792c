"""The stage-wise checker of tests/mlp_checker.py is not vacuous (CPU only).

For every swept shape, with its F1 operands (K = D) and its dW4 operands
(K = M): an f32 CPU matmul passes the derived bound, and a result with its last
16-wide k-chunk, or its last batch-row pair, dropped fails it on at least one
element -- or, where the reduction is so long that the dropped part is of the
size of the bound itself, an exact-arithmetic GPU test covers that GEMM at that
reduction length (``EXACT_D`` / ``EXACT_M``).
"""

import pytest
import torch

from multidisttorch_amd.models.mlp_vae import arena_layout, init_params_, reference_forward, views
from tests import mlp_checker as ck


def _operands(sid, M):
    """x[M, D], W1, b1 and the dW4 operands dlog[M, D], h3[M, H] of an f32 forward."""
    s = ck.SHAPES[sid]
    g = torch.Generator().manual_seed(1000 + M)
    layout, numel, _ = arena_layout(s["D"], s["H"], s["Z"])
    flat = torch.zeros(numel)
    init_params_(flat, layout, g)  # U(+-1/sqrt(fan_in))
    v = views(flat, layout)
    x = torch.rand(M, s["D"], generator=g)
    eps = torch.randn(M, s["Z"], generator=g)
    f = reference_forward(v, x, eps)
    return x, v["fc1.weight"], v["fc1.bias"], f["p"] - x, f["h3"]


def _mutants(A, last_pair_axis):
    """A with its last 16-wide k-chunk zeroed, and with its last batch-row pair zeroed."""
    K = A.shape[1]
    chunk = A.clone()
    chunk[:, 16 * ((K + 15) // 16 - 1):] = 0
    pair = A.clone()
    n = A.shape[last_pair_axis]
    sl = slice(2 * ((n + 1) // 2 - 1), None)
    if last_pair_axis == 0:
        pair[sl] = 0
    else:
        pair[:, sl] = 0
    return {"chunk": chunk, "pair": pair}


@pytest.mark.parametrize("sid,M", ck.cases())
def test_bound_holds_for_f32_matmul_and_catches_mutants(sid, M):
    s = ck.SHAPES[sid]
    x, W1, b1, dlog, h3 = _operands(sid, M)
    gemms = {"F1": (x, W1.t(), b1, 0, s["D"] in ck.EXACT_D)}
    if not s.get("forward_only"):
        gemms["dW4"] = (dlog.t().contiguous(), h3, None, 1, M in ck.EXACT_M)
    for name, (A, B, bias, axis, exact) in gemms.items():
        ref, bound = ck.gemm_ref(A, B, bias)
        got = A @ B if bias is None else A @ B + bias
        r = ck.ratio(got, ref, bound)
        print(f"{sid} M={M} {name}: K={A.shape[1]} f32 matmul error/bound {r:.3f}")
        assert r <= 1.0, (sid, M, name, r)
        for mname, Am in _mutants(A, axis).items():
            bad = Am @ B if bias is None else Am @ B + bias
            frac = ck.outside(bad, ref, bound)
            print(f"{sid} M={M} {name} {mname}-mutant: {100 * frac:.2f}% of outputs outside the bound, "
                  f"exact test: {exact}")
            assert frac > 0 or exact, (sid, M, name, mname)


def test_long_reductions_have_exact_tests():
    """The two cases the bound is known not to catch reliably (a dropped chunk of
    1024 at D = 16384 moves 0.1% of the outputs outside it; a dropped row pair
    of 2048 at M = 4096 is marginal) are in the exact-arithmetic lists, and
    those lists name swept shapes with these reduction lengths."""
    assert ck.SHAPES["img128"]["D"] in ck.EXACT_D
    assert ck.SHAPES["bmax"]["Ms"][0] in ck.EXACT_M
    for D, sid in ck.EXACT_D.items():
        assert ck.SHAPES[sid]["D"] == D
    for M, sid in ck.EXACT_M.items():
        assert M in ck.SHAPES[sid]["Ms"]
    # every swept reduction longer than the default's is covered
    for sid, s in ck.SHAPES.items():
        assert s["D"] <= 896 or s["D"] in ck.EXACT_D, sid
        assert all(m <= 128 or m in ck.EXACT_M or s.get("forward_only") for m in s["Ms"]), sid


def test_checker_rejects_what_it_should():
    """ratio(): an error where the bound is zero, or a non-finite value, never passes."""
    ref = torch.zeros(2, 2, dtype=torch.float64)
    bound = torch.tensor([[0.0, 1e-6], [1e-6, 0.0]], dtype=torch.float64)
    assert ck.ratio(torch.zeros(2, 2), ref, bound) == 0.0
    assert ck.ratio(torch.tensor([[1e-9, 0.0], [0.0, 0.0]]), ref, bound) == float("inf")
    assert ck.ratio(torch.tensor([[0.0, float("nan")], [0.0, 0.0]]), ref, bound) == float("inf")
    assert 0.4 < ck.ratio(torch.tensor([[0.0, 5e-7], [0.0, 0.0]]), ref, bound) < 0.6
    # the exact-data guard: 2^24 + 1 is not an f32 number
    a = torch.tensor([[4096.0, 1.0]])
    assert not ck.exact_ok(a, a.t().contiguous())
    # representable, but a partial sum may not be: 2^24 + 1 - 1
    assert not ck.exact_ok(torch.tensor([[4096.0, 1.0, -1.0]]), torch.tensor([[4096.0], [1.0], [1.0]]))
    assert ck.exact_ok(torch.ones(1, 1024), torch.ones(1024, 1))


# ------------------------------------------------- f32 emulation of one step ----
def emulate(v, x, eps, klw, fb=0.0, mut=None, kn=None):
    """One MLP-VAE step in plain f32 torch -> (stored activations, named gradients, loss), with the knobs of
    tests/knob_cases.py: the free-bits floor (decided on kl_d itself), and with ``kn`` = dict(tc_t, tc_weight)
    the total-correlation share added to d[mu|lv] after the floor decision, before dh1 and the fc21 / fc22
    gradients read it. ``mut`` names one mutation of tests/unit/test_knob_cases.py."""
    import numpy as np

    from tests import tc_cases as tcc

    kn = kn or {}
    Z = v["fc3.weight"].shape[1]
    W2 = torch.cat([v["fc21.weight"], v["fc22.weight"]], 0)
    b2 = torch.cat([v["fc21.bias"], v["fc22.bias"]], 0)
    d = {}
    d["h1"] = torch.relu(x @ v["fc1.weight"].t() + v["fc1.bias"])
    d["mulv"] = d["h1"] @ W2.t() + b2
    mu, lv = d["mulv"][:, :Z], d["mulv"][:, Z:]
    d["eps"] = eps.float()
    sd = torch.exp(0.5 * lv)
    d["z"] = mu + d["eps"] * sd
    d["h3"] = torch.relu(d["z"] @ v["fc3.weight"].t() + v["fc3.bias"])
    t = d["h3"] @ v["fc4.weight"].t() + v["fc4.bias"]
    d["recon"] = torch.sigmoid(t)
    d["dlog"] = d["recon"] - x
    kl = -0.5 * (1 + lv - mu * mu - sd * sd)
    kl_f = np.float32(klw) * kl if mut == "floor_with_klt" else kl
    fl = (kl_f < fb) if fb > 0 else torch.zeros_like(kl, dtype=torch.bool)
    loss = float(ck.bce_terms(t, x).sum() + np.float32(klw) * torch.where(fl, torch.full_like(kl, fb), kl).sum())
    d["dh3"] = (d["dlog"] @ v["fc4.weight"]) * (d["h3"] > 0)
    dz = d["dh3"] @ v["fc3.weight"]
    be = torch.where(fl, torch.zeros_like(dz), torch.full_like(dz, klw))
    pre = torch.cat([dz + be * mu, 0.5 * dz * d["eps"] * sd + 0.5 * be * (sd * sd - 1)], 1)
    d["dmulv"] = pre
    if kn.get("tc_t"):
        tct = kn["tc_weight"] if mut == "tc_no_ramp" else kn["tc_t"]
        add = np.float32(tct) * tcc.oracle(d["mulv"], d["eps"], torch.float32)[1].float()
        if mut == "fold_skips_floored":
            add = add * (~torch.cat([fl, fl], 1))
        d["dmulv"] = pre + add
    d["dh1"] = ((pre if mut == "consumer_prefold" else d["dmulv"]) @ W2) * (d["h1"] > 0)
    gml = pre if mut == "wg_prefold" else d["dmulv"]
    g = {"fc4.weight": d["dlog"].t() @ d["h3"], "fc4.bias": d["dlog"].sum(0),
         "fc3.weight": d["dh3"].t() @ d["z"], "fc3.bias": d["dh3"].sum(0),
         "fc21.weight": gml[:, :Z].t() @ d["h1"], "fc21.bias": gml[:, :Z].sum(0),
         "fc22.weight": gml[:, Z:].t() @ d["h1"], "fc22.bias": gml[:, Z:].sum(0),
         "fc1.weight": d["dh1"].t() @ x, "fc1.bias": d["dh1"].sum(0)}
    return d, g, loss
