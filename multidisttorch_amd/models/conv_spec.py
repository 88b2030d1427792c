"""The conv VAE's definition: layer list, arena layout, accepted latent sizes
and ``TorchConvVAE``, the same network in stock torch ops (fp32, NCHW): the CPU
backend and the numerical oracle of the GPU tests (models/conv_vae.py holds the
trainer)."""

from __future__ import annotations

import math
import operator
from dataclasses import dataclass
from typing import Dict, List

import torch
import torch.nn.functional as F
from torch import nn

from .mlp_vae import free_bits_floor

__all__ = ["Layer", "conv_vae_spec", "TorchConvVAE", "conv_layout", "check_latent_size"]


@dataclass(frozen=True)
class Layer:
    name: str
    kind: str          # conv | convT | linear
    cin: int
    cout: int
    k: int
    s: int
    p: int
    relu: bool
    in_hw: int         # input spatial size (1 for linear)
    out_hw: int


Z_MIN, Z_MAX = 8, 1024


def check_latent_size(z) -> int:
    """The latent sizes ``ConvVaeTrainer`` accepts: multiples of 8 in
    [Z_MIN, Z_MAX], the same on both backends so a configuration never depends
    on the backend. The HIP layer path needs z % 8 == 0: z is the reduction
    length K of the decoder Linear (``plan_fwd`` rejects K % 8 != 0: operands
    are staged in 16-B pieces of 8 bf16) and its weight gradient reads z16
    rows in the same pieces; the head's 2z output channels (``plan_wgrad``:
    CO % 8, the column-sum kernel: N % 8) need only z % 4. The upper end keeps
    every slab offset of the two Linear layers inside int32 at both image
    sizes. See docs/KERNELS.md, "conv-VAE small kernels: domain and checks"."""
    try:
        zi = operator.index(z)
    except TypeError:
        zi = -1
    if not Z_MIN <= zi <= Z_MAX or zi % 8:
        raise ValueError(f"conv-VAE latent size z must be a multiple of 8 in [{Z_MIN}, {Z_MAX}], got {z!r}")
    return zi


def conv_vae_spec(image: int = 28, channels: int = 1, z: int = 32) -> List[Layer]:
    if image == 28:
        enc = [(channels, 32), (32, 64)]
    elif image == 128:
        enc = [(channels, 32), (32, 64), (64, 128), (128, 256)]
    else:
        raise ValueError("image must be 28 or 128")
    L, hw = [], image
    for i, (ci, co) in enumerate(enc):
        L.append(Layer(f"enc{i + 1}", "conv", ci, co, 4, 2, 1, True, hw, hw // 2))
        hw //= 2
    flat = enc[-1][1] * hw * hw
    L.append(Layer("enc_head", "linear", flat, 2 * z, 1, 1, 0, False, 1, 1))
    L.append(Layer("dec_fc", "linear", z, flat, 1, 1, 0, True, 1, 1))
    dec = [(co, ci) for (ci, co) in reversed(enc)]
    for i, (ci, co) in enumerate(dec):
        last = i == len(dec) - 1
        L.append(Layer(f"dec{i + 1}", "convT", ci, co, 4, 2, 1, not last, hw, hw * 2))
        hw *= 2
    return L


def _w_shape(l: Layer):
    """Our weight layout: conv/linear [Cout][K][K][Cin]; convT [Cin_t][K][K][Cout_t]."""
    if l.kind == "convT":
        return (l.cin, l.k, l.k, l.cout)
    return (l.cout, l.k, l.k, l.cin)


def conv_layout(spec: List[Layer]):
    """[(name, offset, shape)], total; weights then bias per layer, 64-aligned."""
    a = lambda v: (v + 63) // 64 * 64
    out, off = [], 0
    for l in spec:
        ws = _w_shape(l)
        out.append((l.name + ".weight", off, ws))
        off = a(off + math.prod(ws))
        out.append((l.name + ".bias", off, (l.cout,)))
        off = a(off + l.cout)
    return out, off


# --------------------------------------------------------------------------
class TorchConvVAE(nn.Module):
    """Reference network in stock torch ops (fp32, NCHW; Linear inputs flattened
    in NHWC order so weights map 1:1 onto the kernel layout)."""

    def __init__(self, spec: List[Layer], image: int, channels: int, z: int):
        super().__init__()
        self.spec, self.image, self.channels, self.z = spec, image, channels, z
        mods = {}
        for l in spec:
            if l.kind == "conv":
                mods[l.name] = nn.Conv2d(l.cin, l.cout, l.k, l.s, l.p)
            elif l.kind == "convT":
                mods[l.name] = nn.ConvTranspose2d(l.cin, l.cout, l.k, l.s, l.p)
            else:
                mods[l.name] = nn.Linear(l.cin, l.cout)
        self.layers = nn.ModuleDict(mods)

    def _run(self, layers, h):
        for l in layers:
            m = self.layers[l.name]
            if l.kind == "linear":
                if h.dim() == 4:  # NCHW -> NHWC flatten
                    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
                h = m(h)
            else:
                if h.dim() == 2:  # NHWC flat -> NCHW
                    c = l.cin
                    hw = int(round(math.sqrt(h.shape[1] // c)))
                    h = h.view(h.shape[0], hw, hw, c).permute(0, 3, 1, 2)
                h = m(h)
            if l.relu:
                h = F.relu(h)
        return h

    def encode(self, x):
        enc = [l for l in self.spec if l.name.startswith("enc")]
        h = self._run(enc, x.view(-1, self.channels, self.image, self.image))
        return h[:, : self.z], h[:, self.z:]

    def decode_logits(self, zz):
        dec = [l for l in self.spec if l.name.startswith("dec")]
        return self._run(dec, zz)

    def forward(self, x, eps):
        mu, lv = self.encode(x)
        zz = mu + eps * torch.exp(0.5 * lv)
        t = self.decode_logits(zz)
        return t, mu, lv

    def loss(self, x, eps, beta: float = 1.0, free_bits: float = 0.0):
        t, mu, lv = self.forward(x, eps)
        xt = x.view(x.shape[0], self.image, self.image, self.channels).permute(0, 3, 1, 2)
        sp_pos = torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
        bce = (xt * torch.clamp(sp_pos - t, max=100.0) + (1 - xt) * torch.clamp(sp_pos, max=100.0)).sum()
        # free bits: floored elements are constants of the objective (no KL gradient through them)
        ksum, _ = free_bits_floor(1 + lv - mu.pow(2) - lv.exp(), free_bits)
        kld = -0.5 * torch.sum(ksum)
        return bce + beta * kld, t, mu, lv

    # weight mapping between torch modules and the kernel arena layout
    def to_arena(self) -> Dict[str, torch.Tensor]:
        out = {}
        for l in self.spec:
            m = self.layers[l.name]
            w = m.weight.detach()
            if l.kind in ("conv", "convT"):
                w = w.permute(0, 2, 3, 1).contiguous()
            else:
                w = w.reshape(l.cout, 1, 1, l.cin)
            out[l.name + ".weight"] = w
            out[l.name + ".bias"] = m.bias.detach()
        return out

    @torch.no_grad()
    def from_arena(self, d: Dict[str, torch.Tensor]):
        for l in self.spec:
            m = self.layers[l.name]
            w = d[l.name + ".weight"].to(m.weight.device, m.weight.dtype)
            if l.kind in ("conv", "convT"):
                m.weight.copy_(w.permute(0, 3, 1, 2))
            else:
                m.weight.copy_(w.reshape(l.cout, l.cin))
            m.bias.copy_(d[l.name + ".bias"])

    def grads_to_arena(self) -> Dict[str, torch.Tensor]:
        out = {}
        for l in self.spec:
            m = self.layers[l.name]
            g = m.weight.grad
            if l.kind in ("conv", "convT"):
                g = g.permute(0, 2, 3, 1).contiguous()
            else:
                g = g.reshape(l.cout, 1, 1, l.cin)
            out[l.name + ".weight"] = g
            out[l.name + ".bias"] = m.bias.grad
        return out
