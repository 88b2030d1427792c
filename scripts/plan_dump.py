#!/usr/bin/env python3
"""Print, as JSON, what the native conv planners decide for a list of geometries
under the CURRENT environment: for each geometry the forward-type plan of both
modes with ``fwd`` and ``allow_split`` off and on, and the weight-gradient plan
(null where the planner rejects the geometry). No GPU needed.

The planner overrides (docs/KNOBS.md, "Planner overrides") are read once per
process, so a sweep runs this once per setting and diffs the outputs:

    MDT_CONV_BM64_BELOW=512 python scripts/plan_dump.py --models --cases > a.json

Geometries: ``--models`` (every layer of the 28x28 and 128x128 conv-VAE at each
``--batches`` size), ``--cases`` (every shape of tests/igemm_cases.py and
tests/direct_cases.py) and any number of ``--desc N,H,W,C,OH,OW,CO,KH,KW,S,P``.
``--root DIR`` imports the package (and the tests' tables) of another checkout,
to compare two trees; ``MDT_NATIVE_SO`` selects another build of one tree.
"""
import argparse
import json
import os
import sys


def _geometries(a):
    out = []
    for s in a.desc:
        d = [int(x) for x in s.split(",")]
        if len(d) != 11:
            raise SystemExit(f"--desc needs 11 ints, got {s!r}")
        out.append(("desc", d))
    if a.models:
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer, conv_vae_spec

        for image in (28, 128):
            for M in a.batches:
                for l in conv_vae_spec(image, 1, 32 if image == 28 else 64):
                    out.append((f"conv{image}.{l.name}.M{M}", list(ConvVaeTrainer._desc(l, M))))
    if a.cases:
        from tests import direct_cases as dc
        from tests import igemm_cases as cs

        for name, _, _, _, sh in cs.fwd_cases():
            out.append((f"igemm.{name}", cs.desc(sh)))
        for cfg, _, sh in cs.SPLITK:
            out.append((f"igemm.splitk{cfg}", cs.desc(sh)))
        for name, _, _, _, sh in cs.wgrad_cases():
            out.append((f"igemm.{name}", cs.desc(sh)))
        out.append(("igemm.job_wgrad", cs.desc(cs.JOB_WGRAD)))
        for name in dc.DIRECT:
            for N in dc.DIRECT_N:
                out.append((f"direct.{name}.N{N}", cs.desc(dc.direct_shape(name, N))))
        for name, (_, H, C, CO, _) in dc.DWGRAD.items():
            for N in dc.DWGRAD_N:
                out.append((f"direct.{name}.N{N}", dc.desc(N, H, H, C, CO)))
        thin = [(32, g) for g in dc.THIN_WGRAD] + dc.THIN_CONV_VALU + dc.THIN_CONV_MFMA
        thin += dc.THIN_TCONV_VALU + dc.THIN_TCONV_PATCH
        for CO, g in thin:
            out.append((f"direct.thin.{dc.gid(CO, g)}", dc.desc(*g, 1, CO)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[1, 7, 64, 128, 256])
    ap.add_argument("--cases", action="store_true")
    ap.add_argument("--desc", action="append", default=[])
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root))
    from multidisttorch_amd.ops import conv_plans as plans

    def ask(f, *args, **kw):
        try:
            return f(*args, **kw)._asdict()
        except RuntimeError:   # "unsupported geometry"
            return None

    rows = []
    for name, d in _geometries(a):
        row = {"name": name, "desc": d, "wgrad": ask(plans.wgrad_plan, d), "igemm": {}}
        for mode in (0, 1):
            for fwd in (False, True):
                for split in (False, True):
                    row["igemm"][f"mode{mode}.fwd{int(fwd)}.split{int(split)}"] = ask(plans.igemm_plan, mode, d, split,
                                                                                      fwd=fwd)
        rows.append(row)
    json.dump(rows, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
