"""tests/direct_cases.py against the real planners (host code, no GPU): every
case reaches the kernel its table names. The direct convs through
``igemm_plan(..., fwd=True)`` (cfg >= 100 with the tile the table states), the
weight gradients through ``wgrad_plan`` (100 DwL1, 101 DwL2, 110 thin_wgrad_k),
the single-channel bodies through ``thin_blocks`` and through ``wgrad_plan`` of
the same geometry, whose cfg is 110 exactly where the host's thin_mfma_geom
holds (the predicate that also selects thin_conv's MFMA body)."""
import os

import pytest

from multidisttorch_amd.ops import conv_plans as plans
from multidisttorch_amd.ops import native
from tests import direct_cases as dc

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


@pytest.fixture(autouse=True)
def _default_forms():
    bad = dc.non_default_env(os.environ)
    if bad:
        pytest.skip(f"non-default kernel switches in the environment: {bad}")


def _C():
    return native.require()


def _mfma_geom(CO, g):
    """thin_mfma_geom as the host evaluates it (through the weight-gradient planner)."""
    N, H, W = g
    return plans.wgrad_plan(dc.desc(N, H, W, 1, CO)).cfg == plans.WG_THIN_MFMA


@pytest.mark.parametrize("name", list(dc.DIRECT))
@pytest.mark.parametrize("N", dc.DIRECT_N)
def test_direct_case_plans_to_its_configuration(name, N):
    cfg, mode, H, C, CO, BM, BN, R, per_img = dc.DIRECT[name]
    q = plans.igemm_plan(mode, dc.desc(N, H, H, C, CO), False, fwd=True)
    assert q.cfg == cfg >= plans.FWD_DIRECT_BASE and (q.bm, q.bn) == (BM, BN), q
    assert q.classes == (1 if mode == dc.CONV else 4)
    assert q.ncols == (CO if mode == dc.CONV else C) and q.k == (16 * C if mode == dc.CONV else 4 * CO)
    assert q.mtiles * q.ntiles == per_img * N              # the grid
    out_rows = H // 2 if mode == dc.CONV else H
    assert q.colsum_rows == N * out_rows // (R if mode == dc.CONV else 2 * R)   # column-sum rows
    # the backward-data call of the same geometry: the 16 <-> 8 tiles are forward only
    back = plans.igemm_plan(mode, dc.desc(N, H, H, C, CO), False).cfg
    assert back == (cfg if cfg < 104 else back) and (cfg < 104 or back < plans.FWD_DIRECT_BASE)


def test_direct_tables_cover_all_six_configurations_and_an_uneven_grid():
    assert sorted(v[0] for v in dc.DIRECT.values()) == [100, 101, 102, 103, 104, 105]
    grids = {v[8] * n for v in dc.DIRECT.values() for n in dc.DIRECT_N}
    assert any(g % 8 for g in grids) and any(g % 8 == 0 for g in grids)
    assert set(dc.DIRECT_JOBS) == {k for k, v in dc.DIRECT.items() if v[0] < 104}


@pytest.mark.parametrize("name", list(dc.DWGRAD))
def test_direct_wgrad_case_plans_to_its_kernel(name, monkeypatch):
    cfg, H, C, CO, l2 = dc.DWGRAD[name]
    if l2:
        monkeypatch.setenv("MDT_DWGRAD_L2", "1")
    else:
        monkeypatch.delenv("MDT_DWGRAD_L2", raising=False)
    for N in dc.DWGRAD_N:
        q = plans.wgrad_plan(dc.desc(N, H, H, C, CO))
        assert q.cfg == cfg and q.nsplit == N and q.mt_per_split == 1, q
    assert {n % 8 == 0 for n in dc.DWGRAD_N} == {True, False}   # both workgroup orders


def test_dwl2_needs_its_switch(monkeypatch):
    monkeypatch.delenv("MDT_DWGRAD_L2", raising=False)
    _, H, C, CO, _ = dc.DWGRAD["DwL2"]
    assert plans.wgrad_plan(dc.desc(3, H, H, C, CO)).cfg < plans.WG_DIRECT_BASE


@pytest.mark.parametrize("g", dc.THIN_WGRAD)
def test_thin_wgrad_case_plans_to_cfg_110(g):
    N, H, W = g
    q = plans.wgrad_plan(dc.desc(N, H, W, 1, 32))
    assert q.cfg == plans.WG_THIN_MFMA and q.nsplit == N * (H // 2) // 4, q


def test_thin_conv_tables_reach_both_bodies_and_every_instantiation():
    C = _C()
    for CO, g in dc.THIN_CONV_VALU:
        assert not dc.thin_mfma_geom(CO, g) and not _mfma_geom(CO, g), (CO, g)
        assert C.thin_blocks(False, dc.desc(*g, 1, CO)) == dc.thin_conv_blocks(g)
    for CO, g in dc.THIN_CONV_MFMA:
        assert dc.thin_mfma_geom(CO, g) and _mfma_geom(CO, g), (CO, g)
        assert C.thin_blocks(False, dc.desc(*g, 1, CO)) == dc.thin_conv_blocks(g) == g[0] * (g[1] // 2) // 4
    assert {co for co, _ in dc.THIN_CONV_VALU} == {16, 32, 64}
    # OW = 64 without the MFMA geometry, a partial block, a tail block across two images
    assert (32, (1, 12, 128)) in dc.THIN_CONV_VALU
    ms = {g[0] * (g[1] // 2) * (g[2] // 2) for _, g in dc.THIN_CONV_VALU}
    assert any(m < 256 for m in ms) and any(m > 256 and m % 256 for m in ms)
    for CO, g, _ in dc.THIN_CONV_GATHER:
        assert (CO, g) in dc.THIN_CONV_VALU + dc.THIN_CONV_MFMA and (g[1] * g[2]) % 4 == 0
    assert {dc.thin_mfma_geom(CO, g) for CO, g, _ in dc.THIN_CONV_GATHER} == {True, False}


def test_thin_tconv_tables_reach_both_forms_and_every_instantiation():
    C = _C()
    for CO, g in dc.THIN_TCONV_VALU:
        assert not dc.tconv_patch_geom(CO, g)
        nb = C.thin_blocks(True, dc.desc(*g, 1, CO))
        assert nb == dc.thin_tconv_blocks(CO, g) and nb % 4 == 0, (CO, g, nb)
    for CO, g in dc.THIN_TCONV_PATCH:
        assert dc.tconv_patch_geom(CO, g)
        assert C.thin_blocks(True, dc.desc(*g, 1, CO)) == dc.thin_tconv_blocks(CO, g) == g[0] * 16
    assert {co for co, _ in dc.THIN_TCONV_VALU} == {16, 32, 64}
    assert (32, (1, 8, 128)) in dc.THIN_TCONV_VALU          # OW = 64 but not square: the VALU body
    for CO, g in dc.THIN_TCONV_OPTIONAL_SHAPES:
        assert (CO, g) in dc.THIN_TCONV_VALU + dc.THIN_TCONV_PATCH
    assert {dc.tconv_patch_geom(CO, g) for CO, g in dc.THIN_TCONV_OPTIONAL_SHAPES} == {True, False}


def test_job_weight_gradient_plans_to_w0():
    from tests import igemm_cases as ics

    assert dc.JOB_WGRAD == ics.JOB_WGRAD and plans.wgrad_plan(ics.desc(dc.JOB_WGRAD)).cfg == 0
