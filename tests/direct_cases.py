"""Case tables of the direct and single-channel conv kernel tests: the
patch-resident direct convs (conv_direct.h: DcS1 DcS2 DcT2 DcT3 DcS3 DcT1), the
direct weight gradient (conv_dwgrad.h: DwL1, DwL2), and the single-channel edge
kernels (conv_thin.h, conv_thin_wg.h: thin_conv and thin_tconv in their VALU,
halo-patch / MFMA forms, thin_wgrad_k).

Shared by tests/unit/test_direct_cases.py (the real planner sends every case to
the kernel it names), tests/unit/test_direct_checker.py (the checker on CPU
emulations) and tests/gpu/test_conv_direct_domain.py (the kernels). Plain data:
no torch at import.

Every geometry is 4x4, stride 2, pad 1 in conv view; ``desc`` gives the 11-int
descriptor [N, H, W, C, OH, OW, CO, 4, 4, 2, 1]. The direct kernels accept one
geometry each (only N varies), so their shapes are the kernels' own; the
single-channel shapes are the smallest that reach each body, tail and edge.
"""

from __future__ import annotations

CONV, PARITY = 0, 1   # kModeConv, kModeTconv


def desc(N, H, W, C, CO):
    return [N, H, W, C, H // 2, W // 2, CO, 4, 4, 2, 1]


# ---- direct conv: name -> (cfg, mode, H, C, CO, BM, BN, R, workgroups per image).
# BM = R x (tile row width) pixels (per parity class in PARITY mode), BN = output
# channels per workgroup; R = output rows (CONV) or class-grid rows (PARITY) per
# workgroup, so a column-sum row covers R (CONV) or 2 R (PARITY) output rows.
DIRECT = {
    "DcS1": (100, CONV, 64, 32, 64, 128, 64, 4, 8),
    "DcS2": (101, CONV, 32, 64, 128, 64, 64, 4, 8),
    "DcT2": (102, PARITY, 32, 64, 128, 64, 32, 4, 8),
    "DcT3": (103, PARITY, 64, 32, 64, 128, 32, 4, 8),
    "DcS3": (104, CONV, 16, 128, 256, 64, 64, 8, 4),   # grid 4 N: odd N takes xcd_remap's remainder branch
    "DcT1": (105, PARITY, 16, 128, 256, 64, 32, 8, 4),
}
DIRECT_N = (1, 3)

# epilogue name -> (bias, relu, mask, colsum, y16, y32)
DIRECT_EPILOGUES = {
    "bias_relu": dict(bias=True, relu=True, mask=False, colsum=False, y16=True, y32=True),
    "mask_colsum": dict(bias=False, relu=False, mask=True, colsum=True, y16=True, y32=True),
    "all_y16": dict(bias=True, relu=True, mask=True, colsum=True, y16=True, y32=False),
    "plain_y32": dict(bias=False, relu=False, mask=False, colsum=False, y16=False, y32=True),
}

# job forms (conv_jobs.hip kCombos): recorded by igemm(job=) as a backward-data
# call next to a W0 weight-gradient job; True = a two-job combination exists
DIRECT_JOBS = {"DcS2": True, "DcT2": True, "DcS1": False, "DcT3": False}
JOB_WGRAD = (5, 14, 8, 72, 4, 2, 1)   # igemm_cases.JOB_WGRAD: plans to W0


def direct_shape(name, N):
    """(N, H, C, CO, k, s, p), the descriptor form of tests/igemm_cases.py."""
    _, _, H, C, CO = DIRECT[name][:5]
    return (N, H, C, CO, 4, 2, 1)


# ---- direct weight gradient: name -> (cfg, H, C, CO, needs MDT_DWGRAD_L2=1)
DWGRAD = {"DwL1": (100, 64, 32, 64, False), "DwL2": (101, 32, 64, 128, True)}
DWGRAD_N = (8, 3, 1)   # XCD-grouped workgroup order (N % 8 == 0), plain order, one image

# ---- thin_wgrad_k (cfg 110): (N, H, W), each with f32 and bf16 X; CO = 32
THIN_WGRAD = [(1, 8, 128), (2, 16, 128)]

# ---- thin_conv, VALU body: (CO, (N, H, W)); none satisfies thin_mfma_geom
_SMALL = [(3, 10, 14), (2, 28, 28)]   # M = 105: one partial block; M = 392: the tail block straddles two images
THIN_CONV_VALU = [(co, g) for co in (16, 32, 64) for g in _SMALL] + [(32, (1, 12, 128))]  # OW = 64, OH % 4 != 0
# ---- thin_conv, MFMA body (CO = 32, W = 128, OH % 4 == 0)
THIN_CONV_MFMA = [(32, (1, 8, 128)), (32, (3, 16, 128))]
THIN_CONV_EPILOGUES = {"bias_relu": dict(bias=True, relu=True, mask=False, colsum=False),
                       "mask_colsum": dict(bias=False, relu=False, mask=True, colsum=True)}
# gather form: (CO, (N, H, W), with hparams)
THIN_CONV_GATHER = [(32, (2, 28, 28), False), (32, (3, 16, 128), True)]

# ---- thin_tconv, VALU body: (CO, (N, H, W)) with H x W the single-channel output
THIN_TCONV_VALU = [(co, g) for co in (16, 32, 64) for g in _SMALL] + [(32, (1, 8, 128))]  # OW = 64, not square
# ---- thin_tconv, halo-patch geometry (the MFMA body under the default MDT_THIN_MFMA)
THIN_TCONV_PATCH = [(32, (1, 128, 128)), (32, (2, 128, 128))]
# optional outputs, as sets of keyword names of C.thin_tconv
THIN_TCONV_OUTPUTS = [("y32",), ("X", "part"), ("X", "part", "gpart", "dlog16"),
                      ("y32", "X", "part", "gpart", "dlog16", "recon")]
THIN_TCONV_OPTIONAL_SHAPES = [(32, (2, 28, 28)), (32, (1, 128, 128))]

# environment switches read once per process into statics: name -> values that leave the default form
ENV_DEFAULTS = {"MDT_THIN_MFMA": ("15",), "MDT_THIN_PATCH": ("1",), "MDT_CONV_DIRECT": ("1",),
                "MDT_DCONV_SMALL": ("1",), "MDT_DWGRAD": ("1",), "MDT_DCONV_BWD": ("1",)}


def non_default_env(environ):
    """Names of the switches above that ``environ`` sets to a non-default value."""
    return sorted(k for k, ok in ENV_DEFAULTS.items() if k in environ and environ[k] not in ok)


def thin_mfma_geom(CO, g):
    N, H, W = g
    return CO == 32 and W == 128 and (H // 2) % 4 == 0


def tconv_patch_geom(CO, g):
    N, H, W = g
    return CO == 32 and H == W == 128


def thin_conv_blocks(g):
    N, H, W = g
    return -(-(N * (H // 2) * (W // 2)) // 256)


def thin_tconv_blocks(CO, g):
    N, H, W = g
    if tconv_patch_geom(CO, g):
        return N * (H // 2) // 4
    return 4 * -(-(N * (H // 2) * (W // 2)) // 256)


def gid(CO, g):
    return f"CO{CO}-N{g[0]}-{g[1]}x{g[2]}"
