"""Shared inputs and bounds of the reconstruction report tests
(tests/unit/test_recon_report.py, tests/gpu/test_recon_kernels.py, tests/gpu/test_recon_gpu.py).

The bound follows tests/tc_cases.py: per column, ``MARGIN`` = 16 times the error
of the oracle (models/recon_report.py) run in float32 against the same oracle in
float64 on the same float32 inputs, floored by one float32 rounding of the
largest value that enters the column: the largest row sum for ``se``, 1 for the
three SSIM columns. It never comes from the code under test.
"""
import torch
import torch.nn.functional as F

from multidisttorch_amd.models import recon_report as rr

MARGIN = 16.0
U32 = 2.0 ** -24  # unit roundoff of float32
NAMES = ("se", "ssim", "l", "cs")


_gen = lambda seed: torch.Generator().manual_seed(seed)


def random(n, S):
    return torch.rand(n, S * S, generator=_gen(1)), torch.rand(n, S * S, generator=_gen(2))


def edge(n, S):
    """A bright block whose corner moves with the row, against its 5-tall, 3-wide
    box blur: the VAE case, different along both axes and off the diagonal."""
    i, y, x = torch.meshgrid(torch.arange(n), torch.arange(S), torch.arange(S), indexing="ij")
    img = torch.where((y > S // 2 + i % 2) & (x > S // 3 + i % 3), 0.9, 0.1)
    blur = F.avg_pool2d(F.pad(img[:, None], (1, 1, 2, 2), mode="replicate"), (5, 3), stride=1)[:, 0]
    return img.reshape(n, -1).contiguous(), blur.reshape(n, -1).contiguous()


def flat(n, S):
    """Constant images, zero variance: rows with x == r and rows with x != r."""
    x = torch.tensor([0.75, 0.75, 1.0, 0.3, 0.0])[torch.arange(n) % 5]
    r = torch.tensor([0.75, 0.25, 0.0, 0.3, 0.0])[torch.arange(n) % 5]
    return x[:, None].expand(n, S * S).contiguous(), r[:, None].expand(n, S * S).contiguous()


def lattice(n, S):
    """Multiples of 1/16: every (x - r)^2 and every partial sum of them is exact in float32."""
    return (torch.randint(0, 17, (n, S * S), generator=_gen(3)) / 16.0,
            torch.randint(0, 17, (n, S * S), generator=_gen(4)) / 16.0)


FAMILIES = dict(random=random, edge=edge, flat=flat, lattice=lattice)


def bounds(real, recon, S):
    """(float64 oracle table, per-column bound [4])."""
    o64 = rr.recon_rows(real.double(), recon.double(), S)
    err = (rr.recon_rows(real, recon, S).double() - o64).abs().amax(0)
    scale = torch.tensor([float(o64[:, 0].max()), 1.0, 1.0, 1.0], dtype=torch.float64)
    return o64, MARGIN * torch.maximum(err, U32 * scale)


def check(got, o64, bound, label):
    """Every row and column of ``got`` within ``bound`` of the oracle; prints error / bound per column."""
    err = (got.detach().cpu().double() - o64).abs().amax(0)
    print(f"recon {label}: " + "  ".join(f"{k} {float(e):.3g}/{float(b):.3g} ({float(e / b) if b > 0 else 0.0:.3f})"
                                         for k, e, b in zip(NAMES, err, bound)))
    assert bool((err <= bound).all()), (label, err.tolist(), bound.tolist())
