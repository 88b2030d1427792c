"""Named results of the native conv planners (``_C.igemm_plan`` / ``_C.wgrad_plan``).

The extension returns its plan structs (``FwdPlan`` / ``WgradPlan`` of
csrc/kernels/conv_igemm.h, filled by conv_plan.hip) as struct sequences made
from one field list; the tuples here are built from them by attribute name, so no
field order is shared with the C++ side. Every reader of a plan in the package,
the tests and the benchmarks goes through this module and reads by name.
"""

from __future__ import annotations

from operator import attrgetter
from typing import NamedTuple

from . import native

__all__ = ["IgemmPlan", "WgradPlan", "igemm_plan", "wgrad_plan", "FWD_DIRECT_BASE", "WG_DIRECT_BASE", "WG_THIN_MFMA"]


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


# each field read from the extension's plan by its NAME, in this tuple's order
_igemm_fields = attrgetter(*IgemmPlan._fields)
_wgrad_fields = attrgetter(*WgradPlan._fields)


def igemm_plan(mode: int, desc, allow_split: bool, fwd: bool = False) -> IgemmPlan:
    return IgemmPlan._make(_igemm_fields(native.require().igemm_plan(mode, desc, allow_split, fwd=fwd)))


def wgrad_plan(desc) -> WgradPlan:
    return WgradPlan._make(_wgrad_fields(native.require().wgrad_plan(desc)))


# The plan numbers (``cfg``) that are no tile index, read from the extension when first asked for:
# FWD_DIRECT_BASE + direct configuration, WG_DIRECT_BASE + DwL index, WG_THIN_MFMA.
def __getattr__(name):
    if name in ("FWD_DIRECT_BASE", "WG_DIRECT_BASE", "WG_THIN_MFMA"):
        return getattr(native.require(), name)
    raise AttributeError(name)
