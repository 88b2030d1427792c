"""Inputs and error bounds of the NDB / k-means tests (models/ndb.py; tests/unit/test_ndb.py,
tests/gpu/test_ndb_kernels.py). The bounds come from the inputs and the oracle alone, never from the kernels.

* distances, the convention of tests/tc_cases.py: MARGIN = 16 times the error of a float32 oracle in the kernels'
  algebraic form (Gram form, x2 + c2 - 2 x.c) against the float64 oracle from differences on the same input,
  floored by one float32 rounding of the largest x2 + c2.
* labels: every case is an input on which the float64 oracle alone decides every row by more than twice that
  bound, at every assignment: ``decide`` raises otherwise. So a kernel within the distance bound has no
  excuse and its labels, counts and ``moved`` must equal the oracle's.
* centroids: MARGIN times the error of the float32 update (``index_add_``, a division) against the float64
  one, floored by one rounding of the largest |x|.
* inertia: MARGIN times the error of the whole fit in float32 Gram form against the float64 one, floored by one
  rounding of x2 + c2 per real row, summed: each row's distance carries one.

Blobs: rows around K random centres in [0, 1]^D with spread 0.05, row i around centre i % K. Uniform: rows in
[0, 1]^D, small K only."""
import torch

from multidisttorch_amd.models import ndb
from tests.latent_cases import MARGIN, U32

# (rows, D, K) of the assign step: rows below one band of 32 and no multiple of it, D no multiple of 4 or of the
# staged chunk of 32, K = 2, a second MFMA tile that is nearly all padding, K = 100, the cap, D = 16384, and the
# smallest row count whose bands are 64 rows high (256 bands of 64)
ASSIGN = [(37, 50, 2), (130, 50, 33), (37, 784, 100), (130, 784, 256), (130, 16384, 33), (16390, 8, 2)]
# (rows, D, K) of the update step: one split; two uneven splits of 1024 rows, a partial second slab of 64 columns;
# the cells of waves' second tiles (K > 128); 17 splits
UPDATE = [(37, 784, 100), (1030, 70, 33), (1030, 20, 256), (16390, 8, 2)]
# (kind, real rows, generated rows, D, K) of the whole fit at T = 5
FIT = [("blobs", 300, 130, 50, 8), ("uniform", 130, 97, 20, 3)]
T_FIT = 5
_cache = {}


def blobs(n, D, K, seed=0):
    """-> (rows float32, the centres float32, the centre of every row)."""
    g = torch.Generator().manual_seed(3000 + seed)
    centres, which = torch.rand(K, D, generator=g), torch.arange(n) % K
    return centres[which] + 0.05 * torch.randn(n, D, generator=g), centres, which


def sqdist64(x, c, block_elems=1 << 23):
    step = max(1, block_elems // (c.shape[0] * c.shape[1]))
    x, c = x.double(), c.double()
    return torch.cat([((x[i: i + step, None] - c[None]) ** 2).sum(2) for i in range(0, x.shape[0], step)])


def gram32(x, c):
    x, c = x.float(), c.float()
    return (x * x).sum(1)[:, None] + (c * c).sum(1)[None] - 2.0 * (x @ c.t())


def decide(x, c):
    """-> (labels, mind, bound) of the float64 oracle for float32 rows and any centroids; raises unless every row's
    best centroid beats the second by more than twice the distance bound."""
    d = sqdist64(x, c)
    scale = float((x.double() ** 2).sum(1).max() + (c.double() ** 2).sum(1).max())
    bound = MARGIN * max(float((gram32(x, c).double() - d).abs().max()), U32 * scale)
    two = d.topk(2, dim=1, largest=False).values
    gap = float((two[:, 1] - two[:, 0]).min())
    if gap <= 2 * bound:
        raise ValueError(f"no case: a row's best two centroids are {gap:.3e} apart, the distance bound is {bound:.3e}")
    return d.argmin(1), two[:, 0], bound


def assign_case(n, D, K):
    """-> dict(x, cent, prev, labels, mind, moved, bound): blobs against the means of their own rows."""
    key = ("assign", n, D, K)
    if key not in _cache:
        x, centres, which = blobs(n, D, K)
        cent = ndb.kmeans_update(x.double(), which, centres.double())[0].float()
        prev = torch.where(torch.arange(n) % 3 == 0, (which + 1) % K, which)
        labels, mind, bound = decide(x, cent)
        _cache[key] = dict(x=x, cent=cent, prev=prev.int(), labels=labels, mind=mind, bound=bound,
                           moved=int((labels != prev).sum()))
    return _cache[key]


def update_case(n, D, K):
    """-> dict(x, labels, cent_in, cent, counts, bound, empty): cell 1 gives its rows to cell 0."""
    key = ("update", n, D, K)
    if key not in _cache:
        x, centres, which = blobs(n, D, K, seed=1)
        labels = torch.where(which == 1, 0, which)
        cent, counts = ndb.kmeans_update(x.double(), labels, centres.double())
        err = float((ndb.kmeans_update(x, labels, centres)[0].double() - cent).abs().max())
        _cache[key] = dict(x=x, labels=labels.int(), cent_in=centres, cent=cent, counts=counts, empty=counts == 0,
                           bound=MARGIN * max(err, U32 * float(x.abs().max())))
    return _cache[key]


def reference(real, fake, init, K, T):
    """-> dict(real, fake, init, labels, moved, inertia, stats, bound): the float64 fit of float32 rows, every
    assignment decided by ``decide``, and the bound of the inertia from the same fit in float32 Gram form."""
    na = real.shape[0]
    c64, c32 = real[init].double(), real[init].clone()
    last, moved = torch.full((na,), -1), []
    for _ in range(T):
        lab = decide(real, c64)[0]
        moved.append(int((lab != last).sum()))
        c64, last = ndb.kmeans_update(real.double(), lab, c64)[0], lab
        c32 = ndb.kmeans_update(real, gram32(real, c32).argmin(1), c32)[0]
    labels, mind, _ = decide(torch.cat([real, fake]), c64)
    inertia = float(mind[:na].sum())
    err = abs(float(gram32(real, c32).min(1).values.clamp(min=0).double().sum()) - inertia)
    floor = U32 * float(((real.double() ** 2).sum(1) + (c64 ** 2).sum(1)[labels[:na]]).sum())
    return dict(real=real, fake=fake, init=init, labels=labels, moved=moved, inertia=inertia,
                stats=ndb.ndb_stats(labels, na, K, inertia, moved[-1], T), bound=MARGIN * max(err, floor))


def fit_case(kind, na, nb, D, K, T=T_FIT):
    """``reference`` of a named input, computed once."""
    key = ("fit", kind, na, nb, D, K, T)
    if key not in _cache:
        if kind == "blobs":
            real, fake = blobs(na, D, K, seed=2)[0], blobs(nb, D, K, seed=3)[0] + 0.02
        else:
            g = torch.Generator().manual_seed(4000)
            real, fake = torch.rand(na, D, generator=g), torch.rand(nb, D, generator=g)
        _cache[key] = reference(real, fake, ndb.ndb_init_idx(na, K, 7), K, T)
    return _cache[key]


def check_stats(got, ref, label):
    """The integers and the divergence of ``ndb_stats`` are the oracle's; the inertia is within its bound."""
    report(label, inertia=abs(got["inertia"] - ref["inertia"]) / ref["bound"])
    assert {k: v for k, v in got.items() if k != "inertia"} == {k: v for k, v in ref["stats"].items() if k != "inertia"}


def report(label, **ratios):
    """Print achieved error / bound per quantity, then assert."""
    print(f"{label}: error/bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
