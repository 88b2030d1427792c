"""Host (numpy) Philox4x32-10 + Box-Muller, bit-identical in its integer part to
``csrc/kernels/common.h`` so the CPU reference path draws the same
reparameterisation noise as the HIP kernels for the same (seed, stream, step).
"""

from __future__ import annotations

import numpy as np

M0 = np.uint64(0xD2511F53)
M1 = np.uint64(0xCD9E8D57)
W0 = np.uint32(0x9E3779B9)
W1 = np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0 = np.asarray(c0, dtype=np.uint32)
    c1 = np.broadcast_to(np.asarray(c1, dtype=np.uint32), c0.shape).copy()
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.uint32), c0.shape).copy()
    c3 = np.broadcast_to(np.asarray(c3, dtype=np.uint32), c0.shape).copy()
    k0 = np.uint32(k0)
    k1 = np.uint32(k1)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = c0.astype(np.uint64) * M0
            p1 = c2.astype(np.uint64) * M1
            lo0 = (p0 & MASK).astype(np.uint32)
            hi0 = (p0 >> np.uint64(32)).astype(np.uint32)
            lo1 = (p1 & MASK).astype(np.uint32)
            hi1 = (p1 >> np.uint64(32)).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0 = np.uint32(k0 + W0)
            k1 = np.uint32(k1 + W1)
    return c0, c1, c2, c3


def normal_from_bits(a, b):
    a = a.astype(np.float32)
    b = b.astype(np.float32)
    u1 = (a + np.float32(1.0)) * np.float32(2.3283064365386963e-10)
    u2 = b * np.float32(2.3283064365386963e-10)
    return (np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.283185307179586) * u2)).astype(np.float32)


def reparam_eps(M: int, Z: int, seed: int, stream: int, step: int) -> np.ndarray:
    """eps[M, Z] exactly as kernel vae_f2 draws it (counter = row*Z + c)."""
    e = np.arange(M * Z, dtype=np.uint64).astype(np.uint32)
    s_lo = np.uint32(step & 0xFFFFFFFF)
    s_hi = np.uint32((step >> 32) & 0xFFFFFFFF)
    x, y, _, _ = philox4x32_10(e, np.uint32(stream), s_lo, s_hi, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return normal_from_bits(x, y).reshape(M, Z)


# Bernoulli resampling of data-set rows (csrc/kernels/binarize.h): the fourth
# counter word of every draw. The reparameterisation noise uses counter
# (e, stream, step_lo, step_hi) under the same key and step_hi = 0 below 2^32
# steps, so a word with non-zero high bits meets none of its draws.
BINARIZE_TAG = 0xB1A50000
BINARIZE_MODES = ("threshold", "static", "dynamic")


def binarize_counter(p: int, row: int, epoch: int, split: int):
    """The Philox counter tuple that serves pixel ``p`` of data-set row ``row``."""
    return (p // 4, int(row) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, BINARIZE_TAG | int(split))


def reparam_counter(e: int, stream: int, step: int):
    """The counter tuple of element ``e`` of ``reparam_eps(.., stream, step)``."""
    return (int(e) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF)


def bernoulli_rows(X, idx, seed: int, epoch: int, split: int, mode: str) -> np.ndarray:
    """``out[i, p] = b(X[idx[i], p])`` as float32 {0, 1}, bit for bit what
    kernel binarize_rows_k writes: ``threshold`` is ``x >= 0.5``; ``static``
    and ``dynamic`` draw ``u < x`` with ``u = (word >> 8) * 2^-24`` from Philox
    counter ``(p // 4, idx[i], epoch, BINARIZE_TAG | split)``, word ``p % 4``
    (``static`` callers pass epoch 0). The conversion and the compare involve
    no rounding, so this is exact, not approximate."""
    if mode not in BINARIZE_MODES:
        raise ValueError(f"unknown binarize mode {mode!r} (one of {', '.join(BINARIZE_MODES)})")
    if split not in (0, 1):
        raise ValueError("split must be 0 (train) or 1 (test)")
    if not 0 <= int(epoch) <= 0xFFFFFFFF:
        raise ValueError("epoch must fit the 32-bit epoch counter word")
    X = np.asarray(X, dtype=np.float32)
    rows = np.asarray(idx).astype(np.int64).reshape(-1)
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("X must be [N, D] with D >= 1")
    if rows.size and (rows.min() < 0 or rows.max() >= X.shape[0]):
        raise IndexError("row index outside the data set")
    x = X[rows]
    if mode == "threshold":
        return (x >= np.float32(0.5)).astype(np.float32)
    n, D = x.shape
    Q = (D + 3) // 4
    q = np.broadcast_to(np.arange(Q, dtype=np.uint32)[None, :], (n, Q))
    r = np.broadcast_to(rows.astype(np.uint32)[:, None], (n, Q))
    w = philox4x32_10(q, r, np.uint32(epoch), np.uint32(BINARIZE_TAG | split), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=-1).reshape(n, 4 * Q)[:, :D]
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u < x).astype(np.float32)
