"""Inputs and error bounds of the sliced Wasserstein tests (models/swd.py; tests/unit/test_swd.py,
tests/gpu/test_swd_kernels.py, test_swd_gpu.py). The bounds come from the inputs and the float64 oracle
alone, never from the kernels.

* lattice inputs: pixels k/16 (sample_cases.lattice), directions m/8 with |m| <= 8, not normalised. Every
  product is a multiple of 1/128 and every partial sum stays below 2^24 / 128 up to D = 16384, so a
  projection is exact in float32 in any order, and so are the sorted values. A table entry then carries the
  rounding of a difference, a square, a product with the segment length, the sum over the na + nb - gcd
  segments and the division: within gamma(na + nb + 4) of the oracle's value.
* uniform inputs, unit directions: a projection is a D-term fma chain, within delta[p, i] = gamma(D)
  sum_c |dirs[p, c]| |x[i, c]|. An order statistic moves by at most the largest change of its arguments, so
  the sorted values are within dmax[p] = max_i delta[p, i] over the union; every difference of the two
  quantile functions then moves by at most 2 dmax, which gives w1 within 2 dmax + gamma(na + nb + 4) w1 and
  w2sq within 4 dmax w1 + 4 dmax^2 + gamma(na + nb + 4) w2sq."""
import torch

from multidisttorch_amd.models import swd
from tests import sample_cases as sc

# (na, nb, D, P): the smallest shapes at which each mechanism of the kernels can go wrong
SHAPES = [
    (2, 2, 1, 1),          # the domain's corner
    (3, 2, 5, 3),          # below one MFMA tile; unequal sets
    (37, 29, 20, 5),       # row, D and P tails; padding 64 / 32
    (130, 257, 33, 33),    # several row tiles, the set boundary inside a tile, P and D one past a tile or chunk
    (128, 128, 784, 32),   # exact tiles, no padding, equal sets
    (64, 48, 16384, 2),    # the long K loop
    (5000, 4100, 8, 2),    # every stage of the sort; pads 8192 / 8192
    (16384, 16383, 2, 2),  # the LDS limit; a full array next to one with a single pad
]
_cache = {}


def case(kind, shape, dup=False):
    """-> (real, fake, dirs, float64 oracle proj, float64 oracle table), computed once. ``dup``: fake = real."""
    key = (kind, shape, dup)
    if key not in _cache:
        na, nb, D, P = shape
        if kind == "lattice":
            real, fake = sc.lattice(na, nb, D)
            dirs = torch.randint(-8, 9, (P, D), generator=torch.Generator().manual_seed(3000)).float() / 8.0
        else:
            real, fake = sc.uniform(na, nb, D)
            dirs = torch.from_numpy(swd.swd_directions(P, D, 11))
        if dup:
            fake = real.clone()
        _cache[key] = (real, fake, dirs) + swd.swd_rows(real.double(), fake.double(), dirs.double())
    return _cache[key]


def float_bounds(real, fake, dirs, table):
    """-> (proj bound [P, 1], table bound [P, 2]) in float64, for float32 inputs and a float64 oracle table."""
    (na, D), nb = real.shape, fake.shape[0]
    dmax = (sc.gamma(D) * (dirs.double().abs() @ torch.cat([real, fake]).double().abs().t())).max(1).values
    g, w1, w2sq = sc.gamma(na + nb + 4), table[:, 0], table[:, 1]
    return dmax[:, None], torch.stack([2 * dmax + g * w1, 4 * dmax * w1 + 4 * dmax ** 2 + g * w2sq], 1)
