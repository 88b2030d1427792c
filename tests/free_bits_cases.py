"""Shared pieces of the free-bits tests (tests/unit/test_free_bits.py,
tests/gpu/test_free_bits_gpu.py): how a test picks its floor, the float64
objective, and the float64 oracles of the two conv-VAE steps with the kernels'
bf16 rounding points, given the mask of floored elements.

The rule under test (csrc/kernels/common.h): the training objective is
``BCE + beta * sum_x sum_d max(fb, kl_d(x))`` with
``kl_d = 0.5 (mu_d^2 + exp(lv_d) - 1 - lv_d)``; an element with ``kl_d < fb`` is
floored: it adds ``fb`` to the KLD sum and its KL gradient is exactly zero.
"""

import torch
import torch.nn.functional as F


def kl_elements(mulv: torch.Tensor, Z: int) -> torch.Tensor:
    """kl_d(x) [M, Z] in float64 from stored [mu | logvar] rows."""
    m = mulv.detach().double().cpu()
    mu, lv = m[:, :Z], m[:, Z:2 * Z]
    return 0.5 * (mu * mu + torch.exp(lv) - 1 - lv)


def choose_floor(kl: torch.Tensor) -> float:
    """The midpoint of the widest gap between consecutive sorted kl_d values
    that lie between the 40th and 60th percentiles: about half the elements
    end up floored, and no element sits near the floor."""
    s = torch.sort(kl.flatten()).values
    n = s.numel()
    lo, hi = int(0.4 * n), max(int(0.6 * n), int(0.4 * n) + 2)
    w = s[lo:hi]
    gaps = w[1:] - w[:-1]
    i = int(torch.argmax(gaps))
    return float(0.5 * (w[i] + w[i + 1]))


def check_floor(kl: torch.Tensor, fb: float, lo: float = 0.3, hi: float = 0.7, margin: float = 1e-4):
    """The conditions on a test's inputs: the share of floored elements and the
    distance of every element from the floor. Returns (reference mask, share)."""
    mask = kl < fb
    share = float(mask.double().mean())
    assert lo <= share <= hi, f"{share:.3f} of the elements floored at fb = {fb}"
    gap = float((kl - fb).abs().min())
    assert gap > margin * fb, f"an element lies within {gap:.3g} of fb = {fb:.6g} (pick another seed)"
    return mask, share


def objective(bce, mu, lv, beta: float, fb: float):
    """BCE + beta * sum max(fb, kl_d), written with torch.clamp (autograd-able)."""
    kl = 0.5 * (mu * mu + torch.exp(lv) - 1 - lv)
    return bce + beta * torch.clamp(kl, min=fb).sum()


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _vjp(fn, inp, wt, gout):
    inp, wt = inp.detach().requires_grad_(), wt.detach().requires_grad_()
    return torch.autograd.grad(fn(inp, wt), (inp, wt), gout)


def _conv(i, w):
    return F.conv2d(i, w, stride=2, padding=1)


def _tconv(i, w):
    return F.conv_transpose2d(i, w, stride=2, padding=1)


def _latent_grads(dz, mu, lv, e, sd, beta, floored):
    """(kld, dm, dl) with the floor: ``floored`` [M, Z] bool or None."""
    ksum = 1 + lv - mu.pow(2) - lv.exp()
    be = torch.full_like(mu, beta)
    kld = -0.5 * ksum
    if floored is not None:
        fl = floored.to(mu.device)
        be = torch.where(fl, torch.zeros_like(be), be)
    dm = dz + be * mu
    dl = 0.5 * dz * e * sd + 0.5 * be * (sd * sd - 1)
    return kld, dm, dl


def _kld_sum(kld, floored, fb):
    if floored is None:
        return kld.sum()
    return torch.where(floored.to(kld.device), torch.full_like(kld, fb), kld).sum()


def _to_arena(tr, g):
    out = {}
    for k, v in g.items():
        if k.endswith(".weight") and v.dim() == 4:
            v = v.permute(0, 2, 3, 1)  # torch [O][I][kh][kw] (convT: [in][out]) -> arena [O][kh][kw][I]
        out[k] = v.reshape(tr.named_grads()[k].shape)
    return out


def emulated_f28(tr, x32, eps, beta=1.0, floored=None, fb=0.0):
    """float64 forward + backward of the fused 28x28 step with its bf16
    rounding points (the construction of tests/gpu/test_conv28_fused.py's
    reference) and the floor applied on ``floored``. Returns (loss, grads)."""
    P = {k: v.detach().double() for k, v in tr.named_parameters().items()}
    W1 = P["enc1.weight"].permute(0, 3, 1, 2)            # f32 master
    W2 = _bf(P["enc2.weight"]).permute(0, 3, 1, 2)
    Wh = _bf(P["enc_head.weight"]).reshape(64, 3136)
    Wd = _bf(P["dec_fc.weight"]).reshape(3136, 32)
    W3 = _bf(P["dec1.weight"]).permute(0, 3, 1, 2)
    W4 = P["dec2.weight"].permute(0, 3, 1, 2)            # f32 master
    b = {k.split(".")[0]: v for k, v in P.items() if k.endswith(".bias")}
    M = x32.shape[0]
    x = x32.double().view(M, 1, 28, 28)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(M, -1)
    nchw = lambda t, c, hw: t.view(M, hw, hw, c).permute(0, 3, 1, 2)
    a1 = _bf(F.relu(_conv(x, W1) + b["enc1"].view(1, -1, 1, 1)))
    a2 = _bf(F.relu(_conv(a1, W2) + b["enc2"].view(1, -1, 1, 1)))
    a2f = nhwc(a2)
    h = a2f @ Wh.t() + b["enc_head"]
    mu, lv = h[:, :32], h[:, 32:]
    e = eps.double()
    sd = torch.exp(0.5 * lv)
    z = _bf(mu + e * sd)
    d0f = _bf(F.relu(z @ Wd.t() + b["dec_fc"]))
    d0 = nchw(d0f, 64, 7)
    d1 = _bf(F.relu(_tconv(d0, W3) + b["dec1"].view(1, -1, 1, 1)))
    t = _tconv(d1, W4) + b["dec2"].view(1, -1, 1, 1)
    sp = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    bce = (x * torch.clamp(sp - t, max=100.0) + (1 - x) * torch.clamp(sp, max=100.0)).sum()
    g = {}
    dlog = torch.sigmoid(t) - x
    gi, _ = _vjp(_tconv, d1, W4, dlog)
    _, g["dec2.weight"] = _vjp(_tconv, d1, W4, _bf(dlog))
    g["dec2.bias"] = dlog.sum().view(1)
    gd1f = gi * (d1 > 0)
    gd1 = _bf(gd1f)
    g["dec1.bias"] = gd1f.sum((0, 2, 3))
    gi, g["dec1.weight"] = _vjp(_tconv, d0, W3, gd1)
    gd0f = nhwc(gi) * (d0f > 0)
    gd0 = _bf(gd0f)
    g["dec_fc.bias"] = gd0f.sum(0)
    dz = gd0 @ Wd
    g["dec_fc.weight"] = gd0.t() @ z
    kld, dm, dl = _latent_grads(dz, mu, lv, e, sd, beta, floored)
    loss = bce + beta * _kld_sum(kld, floored, fb)
    dmulv = torch.cat([dm, dl], 1)
    g["enc_head.bias"] = dmulv.sum(0)
    g["enc_head.weight"] = _bf(dmulv).t() @ a2f
    ga2f = (dmulv @ Wh) * (a2f > 0)
    ga2 = _bf(ga2f)
    g["enc2.bias"] = ga2f.view(M, 49, 64).sum((0, 1))
    gi, g["enc2.weight"] = _vjp(_conv, a1, W2, nchw(ga2, 64, 7))
    ga1f = gi * (a1 > 0)
    ga1 = _bf(ga1f)
    g["enc1.bias"] = ga1f.sum((0, 2, 3))
    _, g["enc1.weight"] = _vjp(_conv, _bf(x), W1, ga1)
    return float(loss), _to_arena(tr, g)


def emulated_layer_path(tr, x32, eps, beta=1.0, floored=None, fb=0.0):
    """float64 forward + backward of the layer-path conv-VAE step (any image
    size) with its rounding points (the construction of
    tests/gpu/test_conv_vae_kernels.py's reference) and the floor applied on
    ``floored``. Returns (loss, grads)."""
    spec, P = tr.spec, {k: v.detach().double() for k, v in tr.named_parameters().items()}
    M = x32.shape[0]
    x = x32.double().view(M, 1, tr.image, tr.image)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(M, -1)

    def W(l):
        w = P[l.name + ".weight"]
        thin = (l is spec[0] and tr._thin_first) or (l is spec[-1] and tr._thin_last)
        w = w if thin else _bf(w)
        return w.permute(0, 3, 1, 2) if w.dim() == 4 else w

    b = {l.name: P[l.name + ".bias"] for l in spec}
    enc = [l for l in spec if l.kind == "conv"]
    head, dfc = [l for l in spec if l.name == "enc_head"][0], [l for l in spec if l.name == "dec_fc"][0]
    dec = [l for l in spec if l.kind == "convT"]
    ins, h = {}, x
    for l in enc:
        ins[l.name] = h
        h = _bf(F.relu(_conv(h, W(l)) + b[l.name].view(1, -1, 1, 1)))
    a_last = h
    flat = nhwc(h)
    mulv = flat @ W(head).reshape(2 * tr.Z, -1).t() + b[head.name]
    mu, lv = mulv[:, :tr.Z], mulv[:, tr.Z:]
    e = eps.double()
    sd = torch.exp(0.5 * lv)
    z = _bf(mu + e * sd)
    d0f = _bf(F.relu(z @ W(dfc).reshape(-1, tr.Z).t() + b[dfc.name]))
    C0, hw = a_last.shape[1], a_last.shape[2]
    h = d0f.view(M, hw, hw, C0).permute(0, 3, 1, 2)
    for l in dec[:-1]:
        ins[l.name] = h
        h = _bf(F.relu(_tconv(h, W(l)) + b[l.name].view(1, -1, 1, 1)))
    last = dec[-1]
    ins[last.name] = h
    t = _tconv(h, W(last)) + b[last.name].view(1, -1, 1, 1)
    sp = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    bce = (x * torch.clamp(sp - t, max=100.0) + (1 - x) * torch.clamp(sp, max=100.0)).sum()
    g = {}
    dlog = torch.sigmoid(t) - x
    g[last.name + ".bias"] = dlog.sum().view(1)
    gcur = _bf(dlog)
    for l in reversed(dec):
        a_in = ins[l.name]
        gi, g[l.name + ".weight"] = _vjp(_tconv, a_in, W(l), gcur)
        gf = gi * (a_in > 0)
        prev = spec[spec.index(l) - 1]
        if prev is dfc:
            gd0 = _bf(nhwc(gf))
            g[dfc.name + ".bias"] = gd0.sum(0)
            gcur = gd0
        else:
            g[prev.name + ".bias"] = gf.sum((0, 2, 3))
            gcur = _bf(gf)
    dz = gcur @ W(dfc).reshape(-1, tr.Z)
    g[dfc.name + ".weight"] = gcur.t() @ z
    kld, dm, dl = _latent_grads(dz, mu, lv, e, sd, beta, floored)
    loss = bce + beta * _kld_sum(kld, floored, fb)
    dmulv16 = _bf(torch.cat([dm, dl], 1))
    g[head.name + ".bias"] = dmulv16.sum(0)
    g[head.name + ".weight"] = dmulv16.t() @ flat
    gaf = (dmulv16 @ W(head).reshape(2 * tr.Z, -1)) * (flat > 0)
    g[enc[-1].name + ".bias"] = gaf.view(M, -1, enc[-1].cout).sum((0, 1))
    gcur = _bf(gaf).view(M, hw, hw, C0).permute(0, 3, 1, 2)
    for l in reversed(enc):
        a_in = ins[l.name]
        gi, g[l.name + ".weight"] = _vjp(_conv, _bf(a_in), W(l), gcur)
        if l is enc[0]:
            break
        gf = gi * (a_in > 0)
        prev = spec[spec.index(l) - 1]
        g[prev.name + ".bias"] = gf.sum((0, 2, 3))
        gcur = _bf(gf)
    return float(loss), _to_arena(tr, g)
