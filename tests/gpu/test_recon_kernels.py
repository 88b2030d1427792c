"""The reconstruction report kernels (csrc/kernels/recon.hip) per row and column
against the float64 oracle on the same float32 inputs (inputs and bounds:
tests/recon_cases.py; no bound comes from the kernels). Sides: one window, 12,
28, the last of the wavefront-per-image kernel (32), the first of the band
kernel (33), two bands of 40 + 14 rows (64), nine (128); 11, 30 and 33 take the
scalar loads. Rows: 1, one more than a workgroup's images, 3 on the band kernel."""
import pytest
import torch

from tests import recon_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = [(11, 1), (11, 5), (12, 5), (28, 1), (28, 5), (30, 5), (32, 5), (33, 3), (64, 3), (128, 3)]


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _rows(real, recon, S, fill):
    C = _C()
    n = real.shape[0]
    ws = torch.zeros(C.recon_ws_numel(n, S), dtype=torch.float32, device=DEV)
    table = torch.zeros(n, C.kReconCols, dtype=torch.float32, device=DEV)
    ws.view(torch.int32).fill_(fill)   # poisoned: nothing unwritten may be read
    table.view(torch.int32).fill_(fill)
    C.recon_rows(real.to(DEV), recon.to(DEV), S, ws, table)
    torch.cuda.synchronize()
    return table.cpu()


@pytest.mark.parametrize("S,n", SHAPES, ids=[f"{S}x{S}-n{n}" for S, n in SHAPES])
@pytest.mark.parametrize("family", list(rc.FAMILIES))
def test_rows_match_the_float64_oracle_and_repeat_bitwise(family, S, n, native_ext):
    C = _C()
    assert (S <= C.kReconWaveSide or n == 3) and (n in (1, 3) or n == C.kReconWaves + 1)
    assert C.recon_bands(S) == {64: 2, 128: 9}.get(S, 1)
    real, recon = rc.FAMILIES[family](n, S)
    o64, bound = rc.bounds(real, recon, S)
    got = _rows(real, recon, S, 0x7FC00000)
    rc.check(got, o64, bound, f"{family} {S}x{S} n={n}")
    assert torch.equal(got, _rows(real, recon, S, -1))
    if family == "lattice":
        assert torch.equal(got[:, 0].double(), o64[:, 0])
    if family == "flat":
        same = (real[:, 0] == recon[:, 0])
        assert bool((got[same, 0] == 0).all()) and bool((got[~same, 0] > 0).all())


@pytest.mark.parametrize("what", ["dtype", "table_shape", "short_ws", "width", "side10", "side257"])
def test_bad_arguments_raise_before_any_launch(what, native_ext):
    C = _C()
    f = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float32), device=DEV)
    a = dict(real=f(3, 64 * 64), recon=f(3, 64 * 64), side=64, ws=f(C.recon_ws_numel(3, 64)), table=f(3, 4))
    bad, err = dict(dtype=(dict(real=f(3, 64 * 64, dtype=torch.float64)), RuntimeError),
                    table_shape=(dict(table=f(3, 3)), RuntimeError), short_ws=(dict(ws=a["ws"][:-1]), RuntimeError),
                    width=(dict(recon=f(3, 64 * 63)), RuntimeError), side10=(dict(side=10), ValueError),
                    side257=(dict(side=257), ValueError))[what]
    with pytest.raises(err):
        C.recon_rows(*[{**a, **bad}[k] for k in ("real", "recon", "side", "ws", "table")])
    C.recon_rows(*a.values())  # the arguments the bad one was derived from are good
    torch.cuda.synchronize()
