"""The sliced Wasserstein kernels (csrc/kernels/swd.hip) against the float64 oracle (models/swd.py, on the
CPU): the sorted projections of every row and direction, and the (w1, w2sq) table. Inputs and bounds:
tests/swd_cases.py; no bound comes from the kernels. Lattice inputs give exact projections, so the sorted
values are compared bit for bit; uniform inputs are held to the fma-chain bound."""
import pytest
import torch

from tests import sample_cases as sc
from tests import swd_cases as wc

pytestmark = pytest.mark.gpu

IDS = ["x".join(map(str, s)) for s in wc.SHAPES]


def _dev():
    return torch.device("cuda", 0)


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _run(real, fake, dirs, fill=0x7FC00000):
    P, n = dirs.shape[0], real.shape[0] + fake.shape[0]
    proj = torch.zeros(P, n, dtype=torch.float32, device=_dev())
    out = torch.zeros(P, 2, dtype=torch.float32, device=_dev())
    proj.view(torch.int32).fill_(fill)   # poisoned: nothing unwritten may be read
    out.view(torch.int32).fill_(fill)
    _C().swd_rows(real.to(_dev()), fake.to(_dev()), dirs.to(_dev()), proj, out)
    torch.cuda.synchronize()
    return proj.cpu(), out.cpu()


@pytest.mark.parametrize("shape", wc.SHAPES, ids=IDS)
def test_lattice_inputs_sorted_projections_exact(shape, native_ext):
    real, fake, dirs, proj, table = wc.case("lattice", shape)
    got_p, got_t = _run(real, fake, dirs)
    bad = (got_p.double() != proj).nonzero()
    assert got_p.shape == proj.shape and bad.numel() == 0, bad[:8].tolist()
    err, bound = (got_t.double() - table).abs(), sc.gamma(shape[0] + shape[1] + 4) * table
    print(f"lattice {shape}: table max error/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert got_t.shape == table.shape and bool((err <= bound).all())


def test_identical_sets_give_exactly_zero(native_ext):
    real, fake, dirs, proj, table = wc.case("lattice", (37, 37, 20, 5), dup=True)
    got_p, got_t = _run(real, fake, dirs)
    assert torch.equal(got_p.double(), proj) and torch.equal(got_t, torch.zeros(5, 2)) and not bool(table.any())


@pytest.mark.parametrize("shape", wc.SHAPES, ids=IDS)
def test_uniform_inputs_within_the_fma_chain_bound(shape, native_ext):
    real, fake, dirs, proj, table = wc.case("uniform", shape)
    pb, tb = wc.float_bounds(real, fake, dirs, table)
    got_p, got_t = _run(real, fake, dirs)
    perr, terr = (got_p.double() - proj).abs(), (got_t.double() - table).abs()
    print(f"uniform {shape}: proj max error/bound {float((perr / pb).max()):.3f} (max error {float(perr.max()):.3e}), "
          f"table {float((terr / tb).max()):.3f} (max error {float(terr.max()):.3e})")
    assert bool((perr <= pb).all()) and bool((terr <= tb).all())


def test_calls_repeat_bitwise(native_ext):
    real, fake, dirs, _, _ = wc.case("uniform", (130, 257, 33, 33))
    a, b = _run(real, fake, dirs), _run(real, fake, dirs, fill=-1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("what", ["dtype", "proj_shape", "out_shape", "rows1", "rows16385", "P0", "P4097"])
def test_bad_arguments_raise_before_any_launch(what, native_ext):
    C = _C()
    assert (C.kSwdMaxRows, C.kSwdMaxDirs) == (16384, 4096)
    f = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float32), device=_dev())
    a = dict(real=f(6, 4), fake=f(5, 4), dirs=f(3, 4), proj=f(3, 11), out=f(3, 2))
    bad, err = dict(dtype=(dict(dirs=f(3, 4, dtype=torch.float64)), RuntimeError),
                    proj_shape=(dict(proj=f(3, 12)), RuntimeError), out_shape=(dict(out=f(3, 3)), RuntimeError),
                    rows1=(dict(fake=f(1, 4)), ValueError), rows16385=(dict(real=f(16385, 4)), ValueError),
                    P0=(dict(dirs=f(0, 4)), ValueError), P4097=(dict(dirs=f(4097, 4)), ValueError))[what]
    with pytest.raises(err):
        C.swd_rows(*{**a, **bad}.values())
    C.swd_rows(*a.values())  # the arguments the bad one was derived from are good
    torch.cuda.synchronize()
