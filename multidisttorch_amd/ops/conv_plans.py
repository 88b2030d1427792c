"""Named results of the native conv planners (``_C.igemm_plan`` / ``_C.wgrad_plan``).

The extension returns plain int lists; their field order is that of the
``info[]`` arrays of ``mdt_igemm_plan`` / ``mdt_wgrad_plan``
(csrc/kernels/conv_igemm.hip:439,449) and is written down here only. A
NamedTuple still indexes, so ``q[10]`` and ``q.ksplit`` are the same read.
"""

from __future__ import annotations

from typing import NamedTuple

from . import native

__all__ = ["IgemmPlan", "WgradPlan", "igemm_plan", "wgrad_plan"]


class IgemmPlan(NamedTuple):
    cfg: int
    bm: int
    bn: int
    classes: int
    m: int
    ncols: int
    k: int
    mtiles: int
    ntiles: int
    ktiles: int
    ksplit: int
    colsum_rows: int


class WgradPlan(NamedTuple):
    cfg: int
    bm: int
    bn: int
    cotiles: int
    ktiles: int
    mtiles: int
    nsplit: int
    mt_per_split: int


def igemm_plan(mode: int, desc, allow_split: bool, fwd: bool = False) -> IgemmPlan:
    return IgemmPlan(*native.require().igemm_plan(mode, desc, allow_split, fwd=fwd))


def wgrad_plan(desc) -> WgradPlan:
    return WgradPlan(*native.require().wgrad_plan(desc))
