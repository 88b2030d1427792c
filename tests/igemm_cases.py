"""Case tables of the conv GEMM tile tests: one shape per tile configuration of
``igemm_fwd_k`` (F0..F7, conv and parity mode, vector and thin gathers) and of
``wgrad_k`` (W0..W5, vector and thin), each the smallest shape with the stated
tails that the DEFAULT planner (``plan_fwd`` / ``plan_wgrad`` of
csrc/kernels/conv_plan.hip, no MDT_CONV_* knob set) sends to that tile.

Shared by tests/unit/test_igemm_tile_cases.py (the real planner returns what
the tables claim), tests/unit/test_igemm_checker.py (the checker at reduced-row
versions) and tests/gpu/test_conv_igemm_tiles.py (the kernels). Plain data: no
torch at import.

Descriptors are ``(N, H, C, CO, k, s, p)`` in conv view (square images), as in
tests/gpu/test_conv_igemm.py: a parity-mode call is the backward-data GEMM of
that conv (rows = input pixels of one stride-parity class, columns = C,
K = (k/s)^2 CO).

Planner thresholds behind the sizes: 128-row tiles need >= 1024 blocks, column
tiles wider than 32 need >= 512 blocks of 64 rows, split-K needs < 256 blocks
and >= 8 k-tiles.
"""

from __future__ import annotations

CONV, PARITY = 0, 1   # kModeConv, kModeTconv

# tile (BM, BN) of forward configuration 0..7 and of weight-gradient configuration 0..5
FWD_TILES = [(128, 128), (128, 64), (128, 32), (128, 16), (64, 128), (64, 64), (64, 32), (64, 16)]
WG_TILES = [(64, 64), (64, 32), (64, 16), (32, 64), (32, 32), (32, 16)]

# ---- forward GEMM, conv mode, vector gathers (bf16 A): (cfg, shape). Per
# configuration a Linear form (1x1 image, K = 136 or 72: the last k-tile is
# partial) and a 4x4 stride-2 form (zero padding, row tail in the last m-tile).
# Every column count leaves a partial last column tile; the 1029-, 2058- and
# 1052-block grids (no multiples of 8) take the uneven branch of xcd_remap.
FWD_CONV_VEC = [
    (0, (16300, 1, 136, 1000, 1, 1, 0)),
    (0, (18, 62, 8, 1000, 4, 2, 1)),
    (1, (131000, 1, 136, 72, 1, 1, 0)),
    (1, (137, 62, 8, 72, 4, 2, 1)),
    (2, (131000, 1, 136, 24, 1, 1, 0)),
    (2, (137, 62, 8, 24, 4, 2, 1)),
    (3, (131000, 1, 72, 8, 1, 1, 0)),
    (3, (137, 62, 8, 8, 4, 2, 1)),
    (4, (4090, 1, 136, 1000, 1, 1, 0)),
    (4, (5, 62, 8, 1000, 4, 2, 1)),
    (5, (32750, 1, 136, 72, 1, 1, 0)),
    (5, (35, 62, 8, 72, 4, 2, 1)),
    (6, (200, 1, 136, 24, 1, 1, 0)),
    (6, (3, 14, 8, 24, 4, 2, 1)),
    (7, (200, 1, 72, 8, 1, 1, 0)),
    (7, (3, 14, 8, 8, 4, 2, 1)),
]

# ---- conv mode, thin (per-element) gathers, C % 8 != 0: run with f32 and with bf16 A
FWD_CONV_THIN = [
    (2, (224, 28, 3, 72, 4, 2, 1)),   # F2, K = 48, 1029 blocks
    (6, (3, 28, 3, 72, 4, 2, 1)),
    (2, (224, 28, 1, 72, 4, 2, 1)),   # F2, K = 16
]

# ---- parity mode: columns = C, K = 4 CO = 96 (the second k-tile is partial)
FWD_PARITY = [
    (0, (6, 62, 1000, 24, 4, 2, 1)),
    (1, (36, 62, 72, 24, 4, 2, 1)),
    (2, (36, 62, 24, 24, 4, 2, 1)),
    (3, (36, 62, 8, 24, 4, 2, 1)),
    (4, (2, 62, 1000, 24, 4, 2, 1)),
    (5, (9, 62, 72, 24, 4, 2, 1)),
    (6, (3, 14, 24, 24, 4, 2, 1)),
    (7, (3, 14, 8, 24, 4, 2, 1)),
]

# ---- split-K with a ragged split (conv mode, a workspace passed): (cfg, ktiles, shape).
# By default only configurations 6 and 7 can split.
SPLITK = [
    (6, 66, (37, 1, 4168, 72, 1, 1, 0)),
    (7, 66, (37, 1, 4168, 8, 1, 1, 0)),
    (6, 18, (70, 1, 1096, 24, 1, 1, 0)),   # the last of 18 k-tiles is partial
]

# ---- weight gradient: (cfg, shape). M is never a multiple of 64, CO = 72 or 24
# leaves a partial last co tile.
WGRAD_VEC = [
    (0, (5, 14, 8, 72, 4, 2, 1)),
    (0, (40, 14, 8, 72, 4, 2, 1)),     # 31 m-tiles in 11 splits of 3: the last split has one tile
    (1, (150, 1, 24, 72, 1, 1, 0)),
    (2, (150, 1, 16, 72, 1, 1, 0)),
    (3, (5, 14, 8, 24, 4, 2, 1)),
    (4, (150, 1, 24, 24, 1, 1, 0)),
    (5, (150, 1, 16, 24, 1, 1, 0)),
]
# thin gathers: run with f32 and with bf16 X
WGRAD_THIN = [
    (0, (5, 14, 3, 72, 4, 2, 1)),
    (2, (5, 14, 1, 72, 4, 2, 1)),
    (3, (5, 14, 3, 24, 4, 2, 1)),
    (5, (5, 14, 1, 24, 4, 2, 1)),
    (5, (5, 14, 1, 24, 3, 1, 1)),      # K2 = 9: the scalar-store epilogue (K2 % 4 != 0)
]

# ---- job forms (conv_jobs.hip kCombos): forward configurations that run as a
# job next to a W0 weight-gradient job, per mode; the others have no job form
JOB_CFGS = {CONV: (1, 4, 5, 6), PARITY: (1, 2, 4, 5, 6)}
JOB_WGRAD = (5, 14, 8, 72, 4, 2, 1)

# every combination the host dispatch can launch (conv_igemm.hip mdt_igemm / mdt_wgrad)
DISPATCHABLE = {
    "conv_vec": set(range(8)), "conv_thin": {2, 6}, "parity": set(range(8)),
    "wgrad_vec": set(range(6)), "wgrad_thin": {0, 2, 3, 5},
}


def desc(shape):
    """The 11-int geometry (N, H, W, C, OH, OW, CO, KH, KW, S, P) of a descriptor."""
    N, H, C, CO, k, s, p = shape
    OH = (H + 2 * p - k) // s + 1
    return [N, H, H, C, OH, OH, CO, k, k, s, p]


def fwd_geom(mode, shape):
    """(classes, M, Ncols, K) of the forward-type GEMM of ``shape`` in ``mode``."""
    N, H, C, CO, k, s, p = shape
    OH = desc(shape)[4]
    if mode == CONV:
        return 1, N * OH * OH, CO, k * k * C
    return s * s, N * (H // s) ** 2, C, (k // s) ** 2 * CO


def with_n(shape, n):
    """The same geometry with ``n`` images: the reduced-row version of a case."""
    return (n,) + tuple(shape[1:])


def reduced(shape, rows=200):
    """A reduced-row version for the CPU checker tests: the fewest images that
    still give >= ``rows`` GEMM rows (so more than one 64- and 128-row tile),
    never more than the case has."""
    OH = desc(shape)[4]
    return with_n(shape, min(shape[0], -(-rows // (OH * OH))))


def fwd_cases():
    """Every forward case as (id, mode, thin, cfg, shape)."""
    out = []
    for cfg, sh in FWD_CONV_VEC:
        out.append((f"conv-F{cfg}-{'lin' if sh[1] == 1 else 'k4s2'}", CONV, False, cfg, sh))
    for cfg, sh in FWD_CONV_THIN:
        out.append((f"thin-F{cfg}-N{sh[0]}-C{sh[2]}", CONV, True, cfg, sh))
    for cfg, sh in FWD_PARITY:
        out.append((f"parity-F{cfg}", PARITY, False, cfg, sh))
    return out


def wgrad_cases():
    """Every weight-gradient case as (id, thin, x_f32, cfg, shape)."""
    out = [(f"vec-W{cfg}-N{sh[0]}", False, False, cfg, sh) for cfg, sh in WGRAD_VEC]
    for cfg, sh in WGRAD_THIN:
        for f32 in (True, False):
            out.append((f"thin-W{cfg}-C{sh[2]}k{sh[4]}-{'f32' if f32 else 'bf16'}", True, f32, cfg, sh))
    return out
