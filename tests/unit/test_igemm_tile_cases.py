"""tests/igemm_cases.py against the real planners (host code, no GPU): every
case plans to the tile configuration its table claims, the tables together
reach every combination the host dispatch can launch, and none of the shapes of
tests/gpu/test_conv_igemm.py's own tables reaches more than F6, F7, W0, W1, W5
-- the gap tests/gpu/test_conv_igemm_tiles.py closes."""
import pytest

from multidisttorch_amd.ops import conv_plans as plans
from multidisttorch_amd.ops import native
from tests import igemm_cases as cs

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


def _fwd(mode, shape, split=False):
    q = plans.igemm_plan(mode, cs.desc(shape), split)
    return dict(cfg=q.cfg, BM=q.bm, BN=q.bn, classes=q.classes, M=q.m, Ncols=q.ncols, K=q.k, mtiles=q.mtiles,
                ntiles=q.ntiles, ktiles=q.ktiles, ksplit=q.ksplit, colsum_rows=q.colsum_rows)


def _wg(shape):
    q = plans.wgrad_plan(cs.desc(shape))
    return dict(cfg=q.cfg, BM=q.bm, BN=q.bn, cotiles=q.cotiles, ktiles=q.ktiles, mtiles=q.mtiles, nsplit=q.nsplit,
                mps=q.mt_per_split)


@pytest.mark.parametrize("name,mode,thin,cfg,shape", cs.fwd_cases(), ids=[c[0] for c in cs.fwd_cases()])
def test_forward_case_plans_to_its_tile(name, mode, thin, cfg, shape):
    q = _fwd(mode, shape)
    assert q["cfg"] == cfg, q
    assert (q["BM"], q["BN"]) == cs.FWD_TILES[cfg]
    assert (q["classes"], q["M"], q["Ncols"], q["K"]) == cs.fwd_geom(mode, shape)
    assert q["ksplit"] == 1
    assert thin == (mode == cs.CONV and shape[2] % 8 != 0)
    # the tails the table promises: partial last row tile and column tile, and a
    # partial last k-tile (the vector 4x4 forms have K = 128: their edge is the zero padding)
    assert q["Ncols"] % q["BN"] and (thin or q["M"] % q["BM"])
    assert q["K"] % 64 or (mode == cs.CONV and not thin and shape[4] == 4 and shape[6] == 1)
    # a workspace would not change the tile, and only F6 / F7 may split
    qs = _fwd(mode, shape, True)
    assert qs["cfg"] == cfg and (qs["ksplit"] == 1 or cfg in (6, 7))


def test_uneven_xcd_grids_are_present():
    grids = {_fwd(m, sh)["mtiles"] * _fwd(m, sh)["ntiles"] for _, m, _, _, sh in cs.fwd_cases()}
    assert {1029, 2058, 1052} <= grids, sorted(grids)   # none a multiple of 8


@pytest.mark.parametrize("cfg,ktiles,shape", cs.SPLITK)
def test_splitk_case_plans_a_ragged_split(cfg, ktiles, shape):
    q = _fwd(cs.CONV, shape, True)
    assert q["cfg"] == cfg and q["ktiles"] == ktiles and q["ksplit"] > 1, q
    assert q["K"] % 64, "the last k-tile is partial"
    assert _fwd(cs.CONV, shape, False)["ksplit"] == 1


@pytest.mark.parametrize("name,thin,x_f32,cfg,shape", cs.wgrad_cases(), ids=[c[0] for c in cs.wgrad_cases()])
def test_wgrad_case_plans_to_its_tile(name, thin, x_f32, cfg, shape):
    q = _wg(shape)
    assert q["cfg"] == cfg and q["cfg"] < 100, q     # never a direct / MFMA-thin weight-gradient kernel
    assert (q["BM"], q["BN"]) == cs.WG_TILES[cfg]
    assert thin == (shape[2] % 8 != 0)
    M = shape[0] * cs.desc(shape)[4] ** 2
    assert M % 64 and shape[3] % q["BM"]
    assert q["nsplit"] == -(-q["mtiles"] // q["mps"])


def test_ragged_wgrad_split():
    q = _wg(cs.WGRAD_VEC[1][1])
    assert (q["mtiles"], q["nsplit"], q["mps"]) == (31, 11, 3), q


def test_scalar_store_case_has_k2_not_multiple_of_4():
    sh = cs.WGRAD_THIN[-1][1]
    assert (sh[4] * sh[4] * sh[2]) % 4 != 0


def test_tables_reach_every_dispatchable_combination():
    got = {k: set() for k in cs.DISPATCHABLE}
    for _, mode, thin, _, sh in cs.fwd_cases():
        key = "parity" if mode == cs.PARITY else "conv_thin" if thin else "conv_vec"
        got[key].add(_fwd(mode, sh)["cfg"])
    for _, thin, _, _, sh in cs.wgrad_cases():
        got["wgrad_thin" if thin else "wgrad_vec"].add(_wg(sh)["cfg"])
    assert got == cs.DISPATCHABLE
    # no forward case is a direct-kernel geometry (cfg >= 100), forward or backward call
    for _, mode, _, _, sh in cs.fwd_cases():
        assert all(plans.igemm_plan(mode, cs.desc(sh), False, f).cfg < plans.FWD_DIRECT_BASE for f in (False, True))


def test_reported_tile_sizes_are_the_tables():
    """Over all cases: every forward configuration 0..7 and weight-gradient
    configuration 0..5 is planned, and the tile the extension reports for it is
    the one FWD_TILES / WG_TILES states."""
    fwd, wg = {}, {}
    for _, mode, _, _, sh in cs.fwd_cases():
        q = _fwd(mode, sh)
        fwd.setdefault(q["cfg"], set()).add((q["BM"], q["BN"]))
    for _, _, _, _, sh in cs.wgrad_cases():
        q = _wg(sh)
        wg.setdefault(q["cfg"], set()).add((q["BM"], q["BN"]))
    assert fwd == {cfg: {tile} for cfg, tile in enumerate(cs.FWD_TILES)}
    assert wg == {cfg: {tile} for cfg, tile in enumerate(cs.WG_TILES)}


def test_special_plan_numbers():
    assert (plans.FWD_DIRECT_BASE, plans.WG_DIRECT_BASE, plans.WG_THIN_MFMA) == (100, 100, 110)


def test_job_table_cases_exist():
    for mode, cfgs in cs.JOB_CFGS.items():
        table = cs.FWD_CONV_VEC if mode == cs.CONV else cs.FWD_PARITY
        assert set(cfgs) <= {c for c, _ in table}
    assert _wg(cs.JOB_WGRAD)["cfg"] == 0


def test_older_kernel_test_tables_reach_only_f6_f7_w0_w1_w5():
    """The finding behind the tile tests: test_conv_igemm.py's three tables
    launch forward configurations 6 and 7 and weight-gradient configurations
    0, 1 and 5 only (its Linear split-K cases are called with a workspace)."""
    from tests.gpu import test_conv_igemm as old

    fwd = {_fwd(cs.CONV, sh, True)["cfg"] for sh in old.CONV_SHAPES}
    fwd |= {_fwd(cs.PARITY, sh, sh[1] == 1)["cfg"] for sh in old.TCONV_SHAPES}
    assert fwd <= {6, 7}, fwd
    assert {_wg(sh[:7])["cfg"] for sh in old.WGRAD_SHAPES} <= {0, 1, 5}
