"""The two-sample kernels (csrc/kernels/two_sample.hip) per element against the
float64 oracle (models/sample_report.py, from differences, on the CPU). Shapes,
inputs and every bound: tests/sample_cases.py -- none comes from the kernels.

* lattice inputs: dmin_r / dmin_f bit for bit, hence every row's real/fake
  decision; the kernel sums within ksum (ULP_EXP u + gamma_n);
* float inputs: dmin_* within delta at the oracle's argmin, the sums within
  sum_j k delta / h plus the lattice terms; decisions are not asserted there;
* one lattice case large enough that a workgroup walks several tiles of its
  strip (sample_cases.LONG_STRIP), one on rows that are not 16-byte aligned;
* two calls bitwise equal, also over a workspace and output pre-filled with NaN
  bits; every bad argument raises before a launch.
Each check prints the largest error / bound ratio it saw.
"""
import pytest
import torch

from tests import sample_cases as sc

pytestmark = pytest.mark.gpu

S = sc.S


def _dev():
    return torch.device("cuda", 0)


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _offset_view(x):
    """x on the device, contiguous, starting one element into its storage: rows not 16-byte aligned."""
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=_dev())
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _rows(real, fake, h, fill=None, prepare=None):
    C = _C()
    na, nb, D = real.shape[0], fake.shape[0], real.shape[1]
    if prepare is not None:
        real, fake = prepare(real), prepare(fake)
    ws = torch.zeros(C.two_sample_ws_numel(na, nb, D), dtype=torch.float32, device=_dev())
    out = torch.zeros(na + nb, C.kTsCols, dtype=torch.float32, device=_dev())
    if fill is not None:
        ws.view(torch.int32).fill_(fill)
        out.view(torch.int32).fill_(fill)
    C.two_sample_rows(real.to(_dev()).contiguous(), fake.to(_dev()).contiguous(), list(h), ws, out)
    torch.cuda.synchronize()
    return out.cpu()


def _check_sums(got, table, bound, what):
    err = (got[:, 2:].double() - table[:, 2:]).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: ksum max error/bound {ratio:.3f} (max error {float(err.max()):.3e})")
    assert bool((err <= bound).all()), (what, ratio)


def _check_lattice(got, c, na, nb, what):
    table = c["table"]
    assert got.shape == (na + nb, 8) and bool(torch.isfinite(got).all())
    assert torch.equal(got[:, :2].double(), table[:, :2]), (got[:, :2].double() - table[:, :2]).abs().max()
    assert torch.equal(got[:, 0] <= got[:, 1], table[:, 0] <= table[:, 1])   # every row, none left out
    _check_sums(got, table, sc.lattice_sum_bound(table, na, nb), what)


LATTICE = [(s, None) for s in sc.SHAPES] + [((37, 29, 20), "fake"), ((37, 29, 20), "real"), ((130, 257, 33), "fake")]


@pytest.mark.parametrize("shape,dup", LATTICE, ids=[f"{s[0]}x{s[1]}x{s[2]}" + (f"-dup{d}" if d else "") for s, d in LATTICE])
def test_lattice_inputs_distances_bitwise_and_every_decision(shape, dup, native_ext):
    c = sc.case("lattice", shape, dup)
    na, nb, _ = shape
    got = _rows(c["real"], c["fake"], c["h"])
    _check_lattice(got, c, na, nb, f"lattice {shape} {dup}")
    if dup == "fake":
        assert float(got[na, 0]) == 0.0 and float(got[1, 1]) == 0.0          # the clamp; the copy counts as real
    if dup == "real":
        assert float(got[0, 0]) == 0.0 == float(got[1, 0])


def test_tile_loop_repeats_inside_a_workgroup(native_ext):
    """Every other shape here runs one tile per workgroup; this one three (sample_cases.LONG_STRIP)."""
    na, nb, _ = sc.LONG_STRIP
    C = _C()
    tiles = -(-(na + nb) // 128)
    strips = C.two_sample_strips(na, nb)
    assert tiles == 100 and strips == 17 and -(-(tiles // 2 + 1) // strips) == 3
    c = sc.case("lattice", sc.LONG_STRIP)
    got = _rows(c["real"], c["fake"], c["h"], fill=-1)
    _check_lattice(got, c, na, nb, f"lattice {sc.LONG_STRIP} three tiles per workgroup")
    assert torch.equal(got, _rows(c["real"], c["fake"], c["h"]))


def test_rows_that_are_not_16_byte_aligned_take_the_scalar_loads(native_ext):
    """D % 4 == 0 alone would choose the 16-byte loads: the bases decide as well."""
    shape = (37, 29, 20)
    c = sc.case("lattice", shape)
    got = _rows(c["real"], c["fake"], c["h"], prepare=_offset_view)
    _check_lattice(got, c, shape[0], shape[1], f"lattice {shape} offset view")
    assert torch.equal(got, _rows(c["real"], c["fake"], c["h"]))   # and bitwise what the aligned rows give


@pytest.mark.parametrize("shape", sc.SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in sc.SHAPES])
def test_float_inputs_within_the_fma_chain_bound(shape, native_ext):
    c = sc.case("uniform", shape)
    na, nb, _ = shape
    got = _rows(c["real"], c["fake"], c["h"])
    table = c["table"]
    dmin_b, ksum_b = sc.float_bounds(c["real"], c["fake"], c["h"], table)
    err = (got[:, :2].double() - table[:, :2]).abs()
    print(f"float {shape}: dmin max error/bound {float((err / dmin_b).max()):.3f} (max error {float(err.max()):.3e})")
    assert bool((err <= dmin_b).all())
    _check_sums(got, table, ksum_b, f"float {shape}")


@pytest.mark.parametrize("shape", [(130, 257, 33), (300, 5, 784)], ids=["130x257x33", "300x5x784"])
def test_calls_repeat_bitwise_and_read_nothing_unwritten(shape, native_ext):
    c = sc.case("uniform", shape)
    a = _rows(c["real"], c["fake"], c["h"])
    assert torch.equal(a, _rows(c["real"], c["fake"], c["h"]))
    for bits in (0x7FC00000, -1):  # quiet NaN, all ones
        assert torch.equal(a, _rows(c["real"], c["fake"], c["h"], fill=bits))
    assert _C().two_sample_strips(*shape[:2]) > 1


def test_strip_count_depends_on_the_rows_alone(native_ext):
    # strips split a row tile's T/2 + 1 column-tile offsets (T tiles of 128 rows); about 2048 workgroups
    C = _C()
    assert C.two_sample_strips(2, 2) == 1 and C.two_sample_strips(300, 5) == 2 and C.two_sample_strips(130, 257) == 3
    assert C.two_sample_strips(10000, 10000) == 12 and C.two_sample_strips(32768, 32768) == 4
    n = C.two_sample_ws_numel(300, 5, 784)   # norms, 2 strips and 1 offset taken both ways, 8 floats per row
    assert n == C.two_sample_ws_numel(300, 5, 1) and 305 + 3 * 305 * 8 <= n <= 305 + 3 * 305 * 8 + 3 * 64


def test_bad_arguments_raise_before_any_launch(native_ext):
    C = _C()
    dev = _dev()
    f = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float32), device=dev)
    h = [1.0, 2.0, 3.0]
    ok = dict(real=f(4, 6), fake=f(3, 6), ws=f(C.two_sample_ws_numel(4, 3, 6)), out=f(7, 8))
    call = lambda **kw: C.two_sample_rows(*[{**ok, **kw}[k] for k in ("real", "fake")], kw.get("h", h),
                                          *[{**ok, **kw}[k] for k in ("ws", "out")])
    for kw in (dict(real=f(1, 6)), dict(fake=f(1, 6)), dict(real=f(32769, 1), fake=f(3, 1)),
               dict(real=f(4, 0), fake=f(3, 0)), dict(real=f(2, 65537), fake=f(2, 65537))):
        with pytest.raises(ValueError):
            call(**kw)
    for fn in (C.two_sample_ws_numel, ):
        for args in ((1, 5, 3), (5, 1, 3), (32769, 5, 3), (5, 32769, 3), (5, 5, 0), (5, 5, 65537)):
            with pytest.raises(ValueError):
                fn(*args)
    for kw in (dict(real=f(4, 6, dtype=torch.float64)), dict(fake=f(3, 6, dtype=torch.bfloat16)),
               dict(real=f(4, 12)[:, ::2]), dict(fake=f(6, 3).t()), dict(fake=f(3, 5)),
               dict(real=torch.zeros(4, 6)), dict(ws=ok["ws"][:-1]), dict(ws=ok["ws"].double()),
               dict(out=f(7, 7)), dict(out=f(8, 8)), dict(out=f(7, 16)[:, ::2]), dict(h=[1.0, 2.0]),
               dict(h=[1.0, 0.0, 2.0]), dict(h=[1.0, float("nan"), 2.0])):
        with pytest.raises(RuntimeError):
            call(**kw)
    call()  # the arguments the bad ones were derived from are good
    torch.cuda.synchronize()
