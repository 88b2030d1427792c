"""Distortion of held-out reconstructions: per-image squared error and SSIM. The oracle.

The test loss mixes the distortion with ``beta * KL`` and, without
``--binarize``, is no likelihood of the grey-level data, so trials of a beta
sweep do not compare on it. The reconstruction report scores the images the
reconstruction PNGs show: each test row ``x`` (``D = S * S`` pixels in [0, 1],
one channel) against ``r = decode(mu(x))``, the Bernoulli mean decoded from the
posterior mean (no noise: the result depends on weights and data only).

Per row, ``COLS = 4`` columns ``se, ssim, l, cs``::

    se = sum_p (x_p - r_p)^2

and, with the normalised 11 x 11 Gaussian window w (sigma 1.5) at the
``(S - 10)^2`` valid positions (Wang et al. 2004; no padding, L = 1)::

    mx = sum w x    my = sum w r
    vx = sum w x^2 - mx^2    vy likewise    vxy = sum w x r - mx my
    l  = (2 mx my + C1) / (mx^2 + my^2 + C1)        C1 = 0.01^2
    cs = (2 vxy + C2) / (vx + vy + C2)              C2 = 0.03^2
    ssim = mean_pos(l * cs)    l = mean_pos(l)    cs = mean_pos(cs)

``l`` falls when a trial loses brightness, ``cs`` when it loses structure (blur).

Everything here is plain torch, dtype-generic (float64 for the tests' oracle);
the trainers' ``torch`` backends run it in float32, and the HIP kernels
(csrc/kernels/recon.hip) compute the same table.
"""

from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

__all__ = ["COLS", "WIN", "SIGMA", "C1", "C2", "MIN_SIDE", "MAX_SIDE", "MAX_ROWS", "check_recon_args", "window",
           "recon_rows", "recon_stats"]

COLS = 4  # a table row: se, ssim, l, cs
WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
MIN_SIDE, MAX_SIDE = WIN, 256
MAX_ROWS = 1 << 20
CHUNK_ELEMS = 1 << 22  # pixels per block of rows: the five stacked maps stay within 80 MiB in float32


def check_recon_args(n: int, D: int) -> int:
    """-> the side S of the ``D = S * S`` pixel images."""
    if int(D) != D or D < 1 or math.isqrt(int(D)) ** 2 != D or not MIN_SIDE <= math.isqrt(int(D)) <= MAX_SIDE:
        raise ValueError(f"the reconstruction report supports square one-channel images of side {MIN_SIDE} to "
                         f"{MAX_SIDE}, got D = {D!r}")
    if int(n) != n or not 1 <= n <= MAX_ROWS:
        raise ValueError(f"the reconstruction report supports 1 <= rows <= {MAX_ROWS}, got {n!r}")
    return math.isqrt(int(D))


def window(dtype=torch.float64, device=None) -> torch.Tensor:
    """The normalised ``[WIN, WIN]`` Gaussian window."""
    k = torch.arange(WIN, dtype=dtype, device=device) - (WIN - 1) / 2
    g = torch.exp(-k * k / (2 * SIGMA ** 2))
    w = g[:, None] * g[None]
    return w / w.sum()


def recon_rows(real: torch.Tensor, recon: torch.Tensor, side: int) -> torch.Tensor:
    """The per-row table ``[n, COLS]`` in the inputs' dtype."""
    n, D = real.shape
    if check_recon_args(n, D) != side or recon.shape != real.shape:
        raise ValueError(f"real {tuple(real.shape)} and recon {tuple(recon.shape)} are not rows of {side} x {side} images")
    w = window(real.dtype, real.device)[None, None]
    out = []
    for i in range(0, n, max(1, CHUNK_ELEMS // D)):
        x = real[i: i + max(1, CHUNK_ELEMS // D)].reshape(-1, 1, side, side)
        r = recon[i: i + x.shape[0]].reshape(-1, 1, side, side)
        mx, my, sxx, syy, sxy = F.conv2d(torch.cat([x, r, x * x, r * r, x * r]), w).chunk(5)
        vx, vy, vxy = sxx - mx * mx, syy - my * my, sxy - mx * my
        l = (2 * mx * my + C1) / (mx * mx + my * my + C1)
        cs = (2 * vxy + C2) / (vx + vy + C2)
        out.append(torch.stack([((x - r) ** 2).sum((1, 2, 3)), (l * cs).mean((1, 2, 3)), l.mean((1, 2, 3)),
                                cs.mean((1, 2, 3))], 1))
    return torch.cat(out)


def recon_stats(table: torch.Tensor, side: int) -> Dict[str, object]:
    """The report of a per-row table, in float64. ``mse`` is the mean per pixel
    over all rows and ``psnr`` is taken of that mean (one perfect row cannot make
    it infinite); the SSIM entries are means over rows, ``ssim_min`` the worst row."""
    t = table.double()
    mse = float(t[:, 0].mean()) / (side * side)
    return dict(rows=int(t.shape[0]), side=int(side), mse=mse, psnr=-10.0 * math.log10(mse) if mse > 0 else math.inf,
                ssim=float(t[:, 1].mean()), ssim_l=float(t[:, 2].mean()), ssim_cs=float(t[:, 3].mean()),
                ssim_min=float(t[:, 1].min()))
