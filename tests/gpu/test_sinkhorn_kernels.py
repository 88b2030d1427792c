"""The Sinkhorn kernels (csrc/kernels/sinkhorn.hip) against the float64 oracle (models/sinkhorn.py, on the
CPU): the three stored cost matrices and m, and the potentials' table with its statistics. Inputs and bounds:
tests/sinkhorn_cases.py; no bound comes from the kernels. Lattice inputs give exact costs, so the matrices
are compared bit for bit and the potentials carry the iterations' error alone."""
import pytest
import torch

from tests import sinkhorn_cases as kc

pytestmark = pytest.mark.gpu

ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


def _dev():
    return torch.device("cuda", 0)


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _poisoned(numel, fill, dtype=torch.float32):
    t = torch.zeros(numel, dtype=dtype, device=_dev())
    t.view(torch.int32).fill_(fill)   # nothing unwritten may be read
    return t


def _cost(real, fake, fill=0x7FC00000):
    C, (na, nb) = _C(), (real.shape[0], fake.shape[0])
    ws, L = _poisoned(C.sinkhorn_ws_numel(na, nb), fill), C.sinkhorn_layout(na, nb)
    C.sinkhorn_cost(real.to(_dev()), fake.to(_dev()), ws)
    torch.cuda.synchronize()
    mat = lambda key, n, ld, cols: ws[L[key]: L[key] + n * ld].view(n, ld)[:, :cols].cpu()
    m = float(ws[L["scale"]: L["scale"] + 2].view(torch.float64)[0])
    return mat("cxy", na, L["ldb"], nb), mat("cxx", na, L["lda"], na), mat("cyy", nb, L["ldb"], nb), m


def _rows(real, fake, E, T, fill=0x7FC00000):
    C, (na, nb) = _C(), (real.shape[0], fake.shape[0])
    ws, pot = _poisoned(C.sinkhorn_ws_numel(na, nb), fill), _poisoned(2 * (na + nb), fill).view(na + nb, 2)
    out = _poisoned(2, fill, torch.float64)
    C.sinkhorn_rows(real.to(_dev()), fake.to(_dev()), E, T, ws, pot, out)
    torch.cuda.synchronize()
    return pot.cpu(), out.cpu()


@pytest.mark.parametrize("shape", kc.COST_SHAPES, ids=ids(kc.COST_SHAPES))
@pytest.mark.parametrize("kind", ["lattice", "uniform"])
def test_costs(kind, shape, native_ext):
    real, fake, (Cxy, Cxx, Cyy, m) = kc.costs(kind, shape)
    *got, gm = _cost(real, fake)
    for name, g, want, bound in zip(("Cxy", "Cxx", "Cyy"), got, (Cxy, Cxx, Cyy), kc.cost_bounds(real, fake)):
        err = (g.double() - want).abs()
        print(f"{kind} {shape} {name}: max error/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert g.shape == want.shape
        if kind == "lattice":
            assert not bool(err.any()), (name, err.nonzero()[:8].tolist())
        else:
            assert bool((err <= bound).all()), name
        if name != "Cxy":   # the mirrored tiles and the diagonal
            assert torch.equal(g, g.t()) and not bool(g.diagonal().any()), name
    if kind == "lattice":
        assert abs(gm - float(m)) <= kc.gamma64(shape[0] ** 2) * float(m)
    else:   # the same double sum over costs that are each within their bound
        assert abs(gm - float(m)) <= float(kc.cost_bounds(real, fake)[1].mean()) + kc.gamma64(shape[0] ** 2) * float(m)


@pytest.mark.parametrize("blur", kc.BLURS, ids=lambda b: f"E{b[0]}-T{b[1]}")
@pytest.mark.parametrize("shape", kc.POT_SHAPES, ids=ids(kc.POT_SHAPES))
def test_lattice_potentials_within_the_float32_oracles_margin_and_bitwise_repeatable(shape, blur, native_ext):
    case = kc.potentials("lattice", shape, *blur)
    pot, out = _rows(case["real"], case["fake"], *blur)
    again = _rows(case["real"], case["fake"], *blur, fill=-1)
    assert torch.equal(pot, again[0]) and torch.equal(out, again[1])
    assert abs(float(out[0]) - case["m"]) <= kc.gamma64(shape[0] ** 2) * case["m"]
    kc.check(pot, out[0], out[1], case, *blur, f"lattice {shape} {blur}")


def test_uniform_potentials_add_the_carried_cost_error(native_ext):
    *shape, E, T = kc.UNIFORM_POT
    case = kc.potentials("uniform", tuple(shape), E, T)
    pot, out = _rows(case["real"], case["fake"], E, T)
    kc.check(pot, out[0], out[1], case, E, T, f"uniform {kc.UNIFORM_POT}")


def test_the_phases_alone_give_the_call(native_ext):
    C, (E, T), case = _C(), kc.BLURS[1], kc.potentials("lattice", kc.POT_SHAPES[1], *kc.BLURS[1])
    real, fake = case["real"].to(_dev()), case["fake"].to(_dev())
    (na, nb), want = (real.shape[0], fake.shape[0]), _rows(real, fake, E, T)
    ws, pot, out = _poisoned(C.sinkhorn_ws_numel(na, nb), -1), _poisoned(2 * (na + nb), -1).view(-1, 2), _poisoned(2, -1, torch.float64)
    C.sinkhorn_cost(real, fake, ws)
    for t in range(T):
        C.sinkhorn_step(na, nb, E, T, t, ws, pot, out)
    torch.cuda.synchronize()
    assert torch.equal(pot.cpu(), want[0]) and torch.equal(out.cpu(), want[1])


@pytest.mark.parametrize("what", ["dtype", "ws_short", "pot_shape", "out_dtype", "rows1", "rows16385", "E0", "Einf", "E4.5",
                                  "T0", "T10001"])
def test_bad_arguments_raise_before_any_launch(what, native_ext):
    C = _C()
    assert (C.kSkCols, C.kSkMaxRows, C.kSkMaxIters) == (2, 16384, 10000)
    f = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float32), device=_dev())
    a = dict(real=f(6, 4), fake=f(5, 4), E=0.05, T=3, ws=f(C.sinkhorn_ws_numel(6, 5)), pot=f(11, 2),
             out=f(2, dtype=torch.float64))
    bad, err = dict(dtype=(dict(fake=f(5, 4, dtype=torch.float64)), RuntimeError),
                    ws_short=(dict(ws=f(C.sinkhorn_ws_numel(6, 5) - 1)), RuntimeError),
                    pot_shape=(dict(pot=f(11, 3)), RuntimeError), out_dtype=(dict(out=f(2)), RuntimeError),
                    rows1=(dict(fake=f(1, 4)), ValueError), rows16385=(dict(real=f(16385, 4)), ValueError),
                    E0=(dict(E=0.0), ValueError), Einf=(dict(E=float("inf")), ValueError), **{"E4.5": (dict(E=4.5), ValueError)},
                    T0=(dict(T=0), ValueError), T10001=(dict(T=10001), ValueError))[what]
    with pytest.raises(err):
        C.sinkhorn_rows(*{**a, **bad}.values())
    C.sinkhorn_rows(*a.values())  # the arguments the bad one was derived from are good
    torch.cuda.synchronize()
