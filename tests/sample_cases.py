"""Inputs, float64 oracle and error bounds of the sample report's tests
(models/sample_report.py; tests/unit/test_sample_report.py on the CPU,
tests/gpu/test_two_sample_kernels.py and test_sample_report_gpu.py on the kernels).

No bound here comes from the code under test. With u = 2^-24 (float32 unit
roundoff) and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, Lemma 3.1):

* lattice inputs (pixels k/16): every product, partial Gram sum, norm and
  q_i + q_j - 2 G is a multiple of 2^-8 below 2^15 up to D = 16384, so d2 is
  exact in float32: dmin_* must equal the float64 oracle bit for bit. A kernel
  sum then carries the error of expf and of n float32 additions:
  ksum (ULP_EXP u + gamma_n), n the number of terms;
* float inputs: d2 = fma(-2, G, fl(q_i + q_j)) with G a D-term fma chain is
  within gamma_{D+2} (q_i + q_j + 2 sum_k |U_ik U_jk|), and the norms add
  gamma_D (q_i + q_j): delta_ij. dmin_* is within delta at the oracle's argmin;
  a kernel sum within sum_j k_s(i,j) delta_ij / h_s plus the lattice terms.

Both sum bounds are relative, which float32 keeps only above 2^-126. Under
gradual underflow an operation whose result is smaller is off by at most one
subnormal spacing, ETA = 2^-149, so each of a sum's n terms adds 3 ETA (expf, its
first-order correction, the addition): kernel values the float64 oracle still
resolves and float32 cannot. This term is a deviation from the bound as first
stated, ksum (ULP_EXP u + gamma_n), and at most 1e-41 per term. The case that
needs it is the uniform (2, 2, 1) corner: with two real rows m is their one
distance, h_0 = m / 4, and a fake row 8.7 times as far away has d2 / h_0 = 306,
a term of 6e-134 that float32 returns as 0.

ULP_EXP: expf is the ROCm device library's (HIP's ``expf``, not ``__expf``); the
HIP programming guide's math-API table gives its maximum error as 1 ulp.
"""
import torch

from multidisttorch_amd.models import sample_report as sr

U = 2.0 ** -24
ULP_EXP = 1.0
ETA = 2.0 ** -149
S = len(sr.BANDWIDTH_SCALES)

# (na, nb, D): the smallest shapes at which each mechanism of the kernels can go wrong
SHAPES = [
    (2, 2, 1),          # the domain's corner
    (3, 2, 5),          # fewer rows than an MFMA tile
    (37, 29, 20),       # row and column tails, D below one K chunk
    (130, 257, 33),     # several row and column tiles, the real/fake boundary inside a tile, D one past a chunk
    (128, 128, 784),    # exact tiles, the workload's D
    (300, 5, 784),      # several strips
    (40, 24, 16384),    # the long K loop
]

# The pair kernel's tile loop repeated inside one workgroup: T = 100 tiles, 51 offsets in 17 strips of 3, so a
# workgroup carries its row state, the staged operands and the LDS images over three tiles, the last strip goes
# from tiles taken both ways (d = 48, 49) to the one at 2 d = T that is not, the real/fake boundary (row 6500)
# lies inside a tile taken both ways and the last tile is partial. D is small: the oracle's cost is N^2 D.
LONG_STRIP = (6500, 6250, 8)

_cache = {}


def gamma(n):
    return n * U / (1.0 - n * U)


def lattice(na, nb, D, seed=0, dup=None):
    """Pixels k/16 in [0, 1]. ``dup``: "fake" makes fake row 0 a copy of real row 1
    (d2 = 0: the clamp and the tie rule), "real" makes real rows 0 and 1 equal."""
    g = torch.Generator().manual_seed(1000 + seed)
    real = torch.randint(0, 17, (na, D), generator=g).float() / 16.0
    fake = torch.randint(0, 17, (nb, D), generator=g).float() / 16.0
    if dup == "fake":
        fake[0] = real[1]
    elif dup == "real":
        real[1] = real[0]
    return real, fake


def uniform(na, nb, D, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.rand(na, D, generator=g), torch.rand(nb, D, generator=g)


def oracle_table(real, fake, h):
    """float64 ``[na + nb, 8]`` from differences, in blocks of about 32 MiB."""
    N, D = real.shape[0] + fake.shape[0], real.shape[1]
    return sr.sample_rows(real.double(), fake.double(), h, chunk=max(1, (1 << 22) // (N * D)))


def case(kind, shape, dup=None):
    """-> dict(real, fake, h, m, table) of a named input, computed once."""
    key = (kind, shape, dup)
    if key not in _cache:
        real, fake = lattice(*shape, dup=dup) if kind == "lattice" else uniform(*shape)
        m = sr.mean_pair_d2(real)
        h = sr.bandwidths_of(m)
        _cache[key] = dict(real=real, fake=fake, m=m, h=h, table=oracle_table(real, fake, h))
    return _cache[key]


def terms(na, nb):
    """[na + nb, 2]: how many j enter a row's real and fake sums (never j = i)."""
    t = torch.tensor([[na, nb]], dtype=torch.float64).repeat(na + nb, 1)
    t[:na, 0] -= 1
    t[na:, 1] -= 1
    return t


def lattice_sum_bound(table, na, nb):
    """[na + nb, 2 S]: ksum (ULP_EXP u + gamma_n) + 3 n ETA."""
    n = terms(na, nb)
    g = ULP_EXP * U + gamma(n)                                  # [N, 2]
    wide = lambda t: torch.cat([t[:, :1].expand(-1, S), t[:, 1:].expand(-1, S)], 1)
    return table[:, 2:] * wide(g) + 3.0 * ETA * wide(n)


def float_bounds(real, fake, h, table):
    """-> (dmin bound [N, 2], ksum bound [N, 2 S]) of float inputs, from the arithmetic alone."""
    na, nb = real.shape[0], fake.shape[0]
    N, D = na + nb, real.shape[1]
    Ud = torch.cat([real, fake]).double()
    q = (Ud * Ud).sum(1)
    qq = q[:, None] + q[None]
    absG = Ud.abs() @ Ud.abs().t()
    delta = gamma(D + 2) * (qq + 2.0 * absG) + gamma(D) * qq     # [N, N]
    d2 = (qq - 2.0 * (Ud @ Ud.t())).clamp_min(0.0)               # only to weigh delta and find the argmin
    eye = torch.eye(N, dtype=torch.bool)
    dm = torch.where(eye, torch.full_like(d2, float("inf")), d2)
    rows = torch.arange(N)
    dmin_b = torch.stack([delta[rows, dm[:, :na].argmin(1)], delta[rows, na + dm[:, na:].argmin(1)]], 1)
    cols = []
    for kind in (slice(0, na), slice(na, N)):
        for hs in h:
            k = torch.where(eye, torch.zeros_like(d2), torch.exp(-d2 / hs))
            cols.append((k * delta / hs)[:, kind].sum(1))
    return dmin_b, torch.stack(cols, 1) + lattice_sum_bound(table, na, nb)


def stat_bounds(table, dmin_b, ksum_b, na, nb):
    """The per-row bounds propagated to the statistics: -> dict of absolute bounds,
    with the accuracies as (lowest, highest) admissible value."""
    r, f = slice(0, na), slice(na, na + nb)
    RRb, RFb = ksum_b[r, :S].sum(0), ksum_b[r, S:].sum(0)
    FRb, FFb = ksum_b[f, :S].sum(0), ksum_b[f, S:].sum(0)
    per = RRb / (na * (na - 1)) + FFb / (nb * (nb - 1)) + 2.0 * RFb / (na * nb)
    RF = table[r, 2 + S:].sum(0)
    gap = table[:, 0] - table[:, 1]
    open_ = gap.abs() <= dmin_b.sum(1)           # rows whose neighbour the error may turn
    real_right = (gap[r] <= 0) & ~open_[r]
    fake_right = (gap[f] > 0) & ~open_[f]
    acc = lambda right, o, n: (int(right.sum()) / n, (int(right.sum()) + int(o.sum())) / n)
    sq = lambda col, b, rows: float((b[rows] / table[rows, col].sqrt().clamp_min(1e-300)).mean())
    return dict(mmd2_per_bandwidth=per, mmd2=float(per.mean()),
                nn_acc_real=acc(real_right, open_[r], na), nn_acc_fake=acc(fake_right, open_[f], nb),
                nn_acc=acc(torch.cat([real_right, fake_right]), open_, na + nb),
                nn_dist_real_to_fake=sq(1, dmin_b[:, 1], r), nn_dist_fake_to_real=sq(0, dmin_b[:, 0], f),
                rf_asym=float(((RFb + FRb) / (RF - RFb)).max()))
