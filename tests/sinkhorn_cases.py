"""Inputs and error bounds of the Sinkhorn divergence tests (models/sinkhorn.py; tests/unit/test_sinkhorn.py,
tests/gpu/test_sinkhorn_kernels.py, test_sinkhorn_gpu.py). The bounds come from the inputs and the oracle
alone, never from the kernels.

* costs, lattice inputs (pixels k/16, sample_cases.lattice): every product, partial Gram sum, norm and
  n_i + n_j - 2 G is a multiple of 2^-8 below 2^15 up to D = 16384, so a cost is exact in float32 in any order:
  the three matrices equal the float64 oracle from differences bit for bit. m is then a sum of exact values
  in double: within gamma(na^2) in double of the oracle's.
* costs, uniform inputs: C = fma(-2, G, fl(n_i + n_j)) with G and the norms fma chains of at most D roundings
  is within gamma(D + 3) (n_i + n_j + 2 |G_ij|); clamping at 0 only moves it towards the true value.
* potentials and statistics, the convention of tests/tc_cases.py: MARGIN = 16 times the error of the same
  oracle run in float32 against the float64 one on the same rows, floored by one float32 rounding of the
  largest value that enters the quantity: the largest |potential| for a potential, ``sinkhorn`` and ``ot``;
  for ``marg_err`` = mean |exp((f - ft) / eps) - 1| the largest |ft| / eps, the size of the terms whose
  difference is exponentiated.
* uniform inputs add the cost error carried through the iterations: a softmin is 1-Lipschitz in the cost in
  the max norm and an averaged step passes on at most half of what the potentials carry, so a potential is
  within (T / 2 + 1) times the largest cost bound on top; ``ot`` adds two potentials' means and ``sinkhorn``
  four, ``marg_err`` exponentiates the difference of two over eps.

The last potentials shape is picked from the iteration kernel's band of 64 rows: 300 rows are five bands,
the last partial, so the merge of the column partials folds several bands."""
import torch

from multidisttorch_amd.models import sinkhorn as sk
from tests import sample_cases as sc
from tests.latent_cases import MARGIN, U32

# (na, nb, D): a ragged tile; several tiles with mirrored off-diagonal ones; D no multiple of the K chunk
COST_SHAPES = [(2, 2, 1), (33, 65, 3), (130, 97, 50), (257, 64, 784)]
POT_SHAPES = [(2, 2, 1), (33, 65, 3), (130, 97, 50), (300, 70, 8)]
# (E, T): only the replacing step; across the end of the anneal; a sharp blur, terms far below the row maximum
BLURS = [(0.5, 1), (0.05, 12), (0.002, 12)]
UNIFORM_POT = (130, 97, 50, 0.05, 12)
_cache = {}


def gamma64(n):
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


def rows(kind, shape):
    return sc.lattice(*shape) if kind == "lattice" else sc.uniform(*shape)


def costs(kind, shape):
    """-> (real, fake, (Cxy, Cxx, Cyy, m) of the float64 oracle), computed once."""
    key = (kind, shape)
    if key not in _cache:
        real, fake = rows(kind, shape)
        _cache[key] = (real, fake, sk.sinkhorn_costs(real.double(), fake.double()))
    return _cache[key]


def cost_bounds(real, fake):
    """-> bounds of (Cxy, Cxx, Cyy) for float inputs: gamma(D + 3) (n_i + n_j + 2 |G_ij|)."""
    x, y = real.double(), fake.double()
    b = lambda u, v: sc.gamma(real.shape[1] + 3) * ((u * u).sum(1)[:, None] + (v * v).sum(1)[None] + 2 * (u @ v.t()).abs())
    return b(x, y), b(x, x), b(y, y)


def reference(real, fake, E, T, exact_costs, c64=None):
    """-> dict(real, fake, pot, m, marg_err, stats: the float64 oracle's; bounds: dict(pot, sinkhorn, ot,
    marg_err)) of float32 rows. ``exact_costs``: float32 holds the rows' costs exactly (lattice inputs)."""
    na = real.shape[0]
    c64 = sk.sinkhorn_costs(real.double(), fake.double()) if c64 is None else c64
    pot, m, merr = sk.sinkhorn_rows(real.double(), fake.double(), E, T, costs=c64)
    p32, m32, e32 = sk.sinkhorn_rows(real, fake, E, T)
    s64, s32 = sk.sinkhorn_stats(pot, na, m, merr, E, T), sk.sinkhorn_stats(p32, na, m32, e32, E, T)
    eps = max(E, 4.0 * 0.5 ** (T - 1)) * float(m)
    top = float(pot.abs().max())
    carried = 0.0 if exact_costs else (T / 2 + 1) * max(float(b.max()) for b in cost_bounds(real, fake))
    bound = lambda err, scale, extra: MARGIN * max(err, U32 * scale) + extra
    bounds = dict(pot=bound(float((p32.double() - pot).abs().max()), top, carried),
                  sinkhorn=bound(abs(s32["sinkhorn"] - s64["sinkhorn"]), top, 4 * carried),
                  ot=bound(abs(s32["ot"] - s64["ot"]), top, 2 * carried),
                  marg_err=bound(abs(s32["marg_err"] - s64["marg_err"]), float(pot[:na, 0].abs().max()) / eps,
                                 2 * carried / eps))
    return dict(real=real, fake=fake, pot=pot, m=float(m), marg_err=float(merr), stats=s64, bounds=bounds)


def potentials(kind, shape, E, T):
    """``reference`` of a named input, computed once."""
    key = (kind, shape, E, T)
    if key not in _cache:
        real, fake, c64 = costs(kind, shape)
        _cache[key] = reference(real, fake, E, T, kind == "lattice", c64)
    return _cache[key]


def check(got_pot, got_m, got_merr, case, E, T, label):
    """Print worst error / bound per quantity, then assert; -> the statistics of the result."""
    na, b, ref = case["real"].shape[0], case["bounds"], case["stats"]
    got = sk.sinkhorn_stats(got_pot, na, got_m, got_merr, E, T)
    ratio = dict(pot=float((got_pot.double().cpu() - case["pot"]).abs().max()) / b["pot"],
                 **{k: abs(got[k] - ref[k]) / b[k] for k in ("sinkhorn", "ot", "marg_err")})
    print(f"{label}: error/bound " + " ".join(f"{k} {v:.3f}" for k, v in ratio.items()) +
          f"; sinkhorn {got['sinkhorn']:.6g} marg_err {got['marg_err']:.3e}")
    assert all(v <= 1.0 for v in ratio.values()), ratio
    return got
