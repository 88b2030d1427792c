"""Error bounds of the PRDC kernels' tests on float inputs (tests/gpu/test_prdc_kernels.py,
test_prdc_gpu.py), from the inputs and the float64 oracle alone.

delta_ij is the bound of sample_cases.float_bounds on a computed d2 = fma(-2, G,
fl(q_i + q_j)). A k-th order statistic moves by at most the largest change of
its arguments, so rad is within max_j delta_ij over the row's own set; dminx is
within delta at the oracle's argmin; a membership d2 <= rad can turn only where
the pair's distance is within delta_ij + the radius bound of the threshold."""
import torch

from tests import sample_cases as sc


def float_bounds(real, fake):
    """-> dict(delta [N, N], rad [N], dminx [N], d2 [N, N]) in float64."""
    na, D = real.shape
    Ud = torch.cat([real, fake]).double()
    N = Ud.shape[0]
    q = (Ud * Ud).sum(1)
    qq = q[:, None] + q[None]
    delta = sc.gamma(D + 2) * (qq + 2.0 * (Ud.abs() @ Ud.abs().t())) + sc.gamma(D) * qq
    same = torch.zeros(N, N, dtype=torch.bool)
    same[:na, :na] = same[na:, na:] = True
    rad_b = torch.where(same & ~torch.eye(N, dtype=torch.bool), delta, torch.zeros_like(delta)).max(1).values
    d2 = torch.cat([((Ud[i0: i0 + 8, None] - Ud[None]) ** 2).sum(-1) for i0 in range(0, N, 8)])
    arg = torch.where(same, torch.full_like(d2, float("inf")), d2).argmin(1)
    return dict(delta=delta, rad=rad_b, dminx=delta[torch.arange(N), arg], d2=d2)


def count_interval(table, na, b):
    """-> (lowest, highest) admissible cnt [N] under thresholds moved by -+(delta_ij + the radius bound)."""
    rad, rad_b = table[:, 0], b["rad"]
    cross, shift = b["d2"][:na, na:], b["delta"][:na, na:]
    in_r = lambda s: cross + s * (shift + rad_b[None, na:]) <= rad[None, na:]   # real row i inside fake j's ball
    in_f = lambda s: cross + s * (shift + rad_b[:na, None]) <= rad[:na, None]   # fake row j inside real i's ball
    return torch.cat([in_r(1).sum(1), in_f(1).sum(0)]), torch.cat([in_r(-1).sum(1), in_f(-1).sum(0)])


def stat_interval(table, na, nb, k, b):
    """-> dict of (lowest, highest) admissible precision, recall, density and coverage."""
    lo, hi = count_interval(table, na, b)
    share = lambda rows: (float((lo[rows] > 0).double().mean()), float((hi[rows] > 0).double().mean()))
    r, f = slice(0, na), slice(na, na + nb)
    gap, open_ = table[r, 2] - table[r, 0], b["dminx"][r] + b["rad"][r]
    cov = (int((gap <= -open_).sum()) / na, int((gap <= open_).sum()) / na)
    return dict(precision=share(f), recall=share(r), coverage=cov,
                density=(float(lo[f].sum()) / (k * nb), float(hi[f].sum()) / (k * nb)))
