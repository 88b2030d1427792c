"""The PRDC kernels (csrc/kernels/prdc.hip) per row against the float64 oracle
(models/prdc.py, from differences, on the CPU). Inputs: tests/sample_cases.py.

* lattice inputs (d2 exact in float32): rad and dminx bit for bit, cnt as
  integers, every row;
* uniform inputs: with delta_ij the bound of sample_cases.float_bounds on a
  computed d2 (recomputed from the inputs, tests/prdc_cases.py), rad within max_j delta_ij over
  the row's own set (a k-th order statistic moves by at most the largest change
  of its arguments), dminx within delta at the oracle's argmin, and cnt inside
  the integer interval that thresholds moved by -+(delta_ij + the radius bound)
  admit, where that interval is narrow (asserted on the oracle first).
No bound comes from the kernels. Each check prints the largest error / bound.
"""
import pytest
import torch

from multidisttorch_amd.models import prdc
from tests import prdc_cases as pc
from tests import sample_cases as sc

pytestmark = pytest.mark.gpu

SHAPES = [(9, 9, 5), (37, 29, 1), (37, 29, 20), (130, 257, 33), (128, 128, 784), (40, 24, 16384)]
# 40 and 33 row tiles in 20 strips: two column tiles per strip in both sets, and in the membership kernel
STRIPS = (5000, 4100, 8)
_oracle = {}


def _dev():
    return torch.device("cuda", 0)


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _case(kind, shape, k, dup=None):
    """-> (real, fake, float64 oracle table), computed once."""
    key = (kind, shape, k, dup)
    if key not in _oracle:
        real, fake = sc.lattice(*shape, dup=dup) if kind == "lattice" else sc.uniform(*shape)
        chunk = max(1, (1 << 22) // (max(shape[:2]) * shape[2]))
        _oracle[key] = (real, fake, prdc.prdc_rows(real.double(), fake.double(), k, chunk=chunk))
    return _oracle[key]


def _rows(real, fake, k, fill=0x7FC00000):
    C = _C()
    na, nb, D = real.shape[0], fake.shape[0], real.shape[1]
    ws = torch.zeros(C.prdc_ws_numel(na, nb, D, k), dtype=torch.float32, device=_dev())
    out = torch.zeros(na + nb, C.kPrdcCols, dtype=torch.float32, device=_dev())
    ws.view(torch.int32).fill_(fill)   # poisoned: nothing unwritten may be read
    out.view(torch.int32).fill_(fill)
    C.prdc_rows(real.to(_dev()), fake.to(_dev()), k, ws, out)
    torch.cuda.synchronize()
    return out.cpu()


def _assert_exact(got, table):
    assert got.shape == table.shape and bool(torch.isfinite(got).all())
    for c, name in enumerate(("rad", "cnt", "dminx")):
        bad = (got[:, c].double() != table[:, c]).nonzero().flatten()
        assert bad.numel() == 0, (name, bad[:8].tolist(), got[bad[:8], c].tolist(), table[bad[:8], c].tolist())


LATTICE = ([(s, k, None) for s in SHAPES for k in (1, 3, 8)] + [((2, 2, 1), 1, None)] +
           [((37, 29, 20), 1, "fake"), ((37, 29, 20), 1, "real")])


@pytest.mark.parametrize("shape,k,dup", LATTICE,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-k{k}" + (f"-dup{d}" if d else "") for s, k, d in LATTICE])
def test_lattice_inputs_every_row_exact(shape, k, dup, native_ext):
    real, fake, table = _case("lattice", shape, k, dup)
    got = _rows(real, fake, k)
    _assert_exact(got, table)
    if dup == "fake":   # d2 = 0 across the sets: the clamp, and inside every radius
        assert float(got[shape[0], 2]) == 0.0 == float(got[1, 2]) and float(got[1, 1]) >= 1
    if dup == "real":   # a zero radius at k = 1 still holds the row's twin, and only a distance of 0
        assert float(got[0, 0]) == 0.0 == float(got[1, 0])


def test_strips_and_tile_loops_in_both_kernels(native_ext):
    na, nb, _ = STRIPS
    strips = _C().prdc_strips(na, nb)
    assert strips > 1 and all(-(-(-(-n // 128)) // strips) > 1 for n in (na, nb))   # tiles per strip, either set
    real, fake, table = _case("lattice", STRIPS, 5)
    got = _rows(real, fake, 5, fill=-1)
    _assert_exact(got, table)
    assert torch.equal(got, _rows(real, fake, 5))


def _float_bounds(shape):
    if ("bounds", shape) not in _oracle:
        _oracle["bounds", shape] = pc.float_bounds(*sc.uniform(*shape))
    return _oracle["bounds", shape]


@pytest.mark.parametrize("shape,k", [(s, k) for s in SHAPES[2:] for k in (1, 3, 8)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_float_inputs_within_the_fma_chain_bound(shape, k, native_ext):
    real, fake, table = _case("uniform", shape, k)
    b = _float_bounds(shape)
    counts = shape[2] <= 33
    if counts:   # on the oracle alone, before the kernels: the open part of the counts is small
        lo, hi = pc.count_interval(table, shape[0], b)
        assert float((hi - lo).sum()) <= 0.02 * float(table[:, 1].sum())
    got = _rows(real, fake, k).double()
    for c, name in ((0, "rad"), (2, "dminx")):
        err = (got[:, c] - table[:, c]).abs()
        print(f"float {shape} k={k}: {name} max error/bound {float((err / b[name]).max()):.3f} (max error {float(err.max()):.3e})")
        assert bool((err <= b[name]).all()), name
    if counts:
        print(f"float {shape} k={k}: cnt open {int((hi - lo).sum())} of {int(table[:, 1].sum())}")
        assert bool(((lo <= got[:, 1]) & (got[:, 1] <= hi)).all())


def test_calls_repeat_bitwise(native_ext):
    real, fake, _ = _case("uniform", (130, 257, 33), 3)
    assert torch.equal(_rows(real, fake, 3), _rows(real, fake, 3, fill=-1))


@pytest.mark.parametrize("what", ["dtype", "out_shape", "short_ws", "k0", "k9", "rows_eq_k"])
def test_bad_arguments_raise_before_any_launch(what, native_ext):
    C = _C()
    f = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float32), device=_dev())
    a = dict(real=f(6, 4), fake=f(5, 4), k=3, ws=f(C.prdc_ws_numel(6, 5, 4, 3)), out=f(11, 3))
    bad, err = dict(dtype=(dict(real=f(6, 4, dtype=torch.float64)), RuntimeError),
                    out_shape=(dict(out=f(11, 4)), RuntimeError), short_ws=(dict(ws=a["ws"][:-1]), RuntimeError),
                    k0=(dict(k=0), ValueError), k9=(dict(k=9), ValueError), rows_eq_k=(dict(fake=f(3, 4)), ValueError))[what]
    with pytest.raises(err):
        C.prdc_rows(*[{**a, **bad}[n] for n in ("real", "fake", "k", "ws", "out")])
    C.prdc_rows(*a.values())  # the arguments the bad one was derived from are good
    torch.cuda.synchronize()
