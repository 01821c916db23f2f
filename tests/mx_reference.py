"""Host model of the block-scaled FP8 / MXFP4 probe kernels (``ops/csrc/gpu_probe_mx.h``), in numpy.

Written from the formats' definitions and the formulas the probe states, not by calling the
library: the OCP ``e4m3fn`` and ``e2m1`` decoders, the E8M0 scale, the public memory layout
(FP4 two elements per byte, the even k in the low nibble; one scale byte per 32 consecutive k
of a row), the probe's operand and scale families and their 15 × 21 table of expected values.
Everything is integer arithmetic or float64 on dyadic numbers far inside 53 bits, so the GPU
tests compare bit-exactly.
"""

import numpy as np

FP8, FP4 = 0, 4  # the hardware's format codes
NAMES = {"fp8": FP8, "fp4": FP4}
ROWS, COLS = 15, 21

FP4_VALUES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=np.float64)


def decode_fp8(codes):
    """OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; 0x7f / 0xff are NaN."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7).astype(np.float64))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(c & 0x80, -mag, mag)


def decode_fp4(packed):
    """e2m1, two per byte: element 2b in the low nibble of byte b, element 2b + 1 in the high."""
    p = np.asarray(packed, dtype=np.uint8)
    nib = np.stack([p & 15, p >> 4], axis=-1).reshape(*p.shape[:-1], p.shape[-1] * 2).astype(np.int64)
    return np.where(nib & 8, -1.0, 1.0) * FP4_VALUES[nib & 7]


def decode(fmt, codes):
    return decode_fp4(codes) if fmt == FP4 else decode_fp8(codes)


def encode(fmt, values):
    """Codes of exactly representable ``values`` ([rows, K]) in the public layout."""
    v = np.asarray(values, dtype=np.float64)
    if fmt == FP8:
        lut = {float(x): c for c, x in enumerate(decode_fp8(np.arange(256))) if x == x and not (c == 0x80)}
        return np.vectorize(lambda x: lut[float(x)], otypes=[np.uint8])(v)
    lut = {float(s * x): (8 if s < 0 else 0) | i
           for i, x in enumerate(FP4_VALUES) for s in (1, -1) if not (s < 0 and i == 0)}
    nib = np.vectorize(lambda x: lut[float(x)], otypes=[np.uint8])(v)
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).astype(np.uint8)


def scale_values(scales):
    """E8M0 bytes → 2^(byte - 127)."""
    return 2.0 ** (np.asarray(scales, dtype=np.int64) - 127).astype(np.float64)


def scaled(fmt, codes, scales):
    """The operand a block-scaled GEMM multiplies: decoded values times their block's scale."""
    return decode(fmt, codes) * np.repeat(scale_values(scales), 32, axis=-1)


def product(fmt, a, bt, sa, sbt):
    return scaled(fmt, a, sa) @ scaled(fmt, bt, sbt).T


# ------------------------------------------------------------------ the probe's operands


def probe_values(m, n, k):
    """``A[i][k] = ((3i + 7k) mod 5) - 2`` and ``Bt[j][k] = ((11j + 5k) mod 7) - 3``."""
    kk = np.arange(k, dtype=np.int64)[None, :]
    a = (3 * np.arange(m, dtype=np.int64)[:, None] + 7 * kk) % 5 - 2
    bt = (11 * np.arange(n, dtype=np.int64)[:, None] + 5 * kk) % 7 - 3
    return a, bt


def probe_scales(rows, k):
    """``s[r][kb] = 126 + (r + kb) mod 3``: 2^-1, 1 and 2."""
    return (126 + (np.arange(rows)[:, None] + np.arange(k // 32)[None, :]) % 3).astype(np.uint8)


def probe_table(k):
    """The 15 × 21 table ``t`` with ``C[i][j] = t[i mod 15][j mod 21]``: A has period 5 in i and
    its scale period 3, Bt period 7 in j and its scale period 3.  Computed in integers, × 4."""
    a, bt = probe_values(ROWS, COLS, k)
    ea = np.repeat((np.arange(ROWS)[:, None] + np.arange(k // 32)[None, :]) % 3, 32, axis=1)
    eb = np.repeat((np.arange(COLS)[:, None] + np.arange(k // 32)[None, :]) % 3, 32, axis=1)
    t4 = (a << ea) @ (bt << eb).T
    return t4 / 4.0


def zero_classes(k):
    if k <= 0 or k % 128:
        return -1
    return int((probe_table(k) == 0).sum())


# ------------------------------------------------------------------ one-hot cases of the store kernel
#
# Each row of A holds one non-zero code and Bt one code throughout, so every output is a single
# product (plus exact zeros): exact whatever order or width the hardware sums in.  The expected
# values come from the formats' definitions, element by element; ``product`` (the matrix
# product of the decoded, scaled operands) must agree, which ``test_probe_mx.py`` checks.

ALL_CODES_M = ALL_CODES_N = 256
SCALE_LO, SCALE_HI = 119, 135  # seeded scales of the one-hot cases: 2^-8 .. 2^8


def all_codes_case(fmt):
    """Every code of ``fmt`` against every code, 256 × 256 at one stage (K = 64 FP8, 128 FP4).

    FP8: ``A[i][k]`` is code ``i`` at ``k = i % 64`` and ``0x00`` elsewhere, ``Bt[j][k]`` is code
    ``j`` at every k.  FP4: nibble code ``i % 16`` (-0, code 8, included) at ``k = i % 128``, and
    ``Bt[j]`` is nibble ``j % 16`` throughout.  Scales are seeded per row and block in 119 .. 135.
    Returns ``a, bt, sa, sbt, want`` with ``want[i][j] = decode(i) · decode(j) · 2^(sA + sBt - 254)``
    of the block that holds row i's element; rows and columns of the FP8 codes 0x7f and 0xff
    are NaN."""
    m, n = ALL_CODES_M, ALL_CODES_N
    i, j = np.arange(m), np.arange(n)
    rng = np.random.default_rng(20240 + fmt)
    if fmt == FP8:
        k = 64
        hot = i % k
        a = np.zeros((m, k), dtype=np.uint8)
        a[i, hot] = i
        bt = np.repeat(j.astype(np.uint8)[:, None], k, axis=1)
        da, db = decode_fp8(i), decode_fp8(j)
    else:
        k = 128
        hot = i % k
        a = np.zeros((m, k // 2), dtype=np.uint8)
        a[i, hot // 2] = (i % 16) << (4 * (hot & 1))
        bt = np.repeat(((j % 16) * 0x11).astype(np.uint8)[:, None], k // 2, axis=1)
        sign = np.where(np.arange(16) & 8, -1.0, 1.0)
        da, db = (sign * FP4_VALUES[np.arange(16) & 7])[i % 16], (sign * FP4_VALUES[np.arange(16) & 7])[j % 16]
    sa = rng.integers(SCALE_LO, SCALE_HI + 1, size=(m, k // 32), dtype=np.uint8)
    sbt = rng.integers(SCALE_LO, SCALE_HI + 1, size=(n, k // 32), dtype=np.uint8)
    blk = hot // 32
    e = sa[i, blk].astype(np.int64)[:, None] + sbt[:, blk].astype(np.int64).T - 254  # [i][j]
    want = da[:, None] * db[None, :] * 2.0 ** e.astype(np.float64)
    return a, bt, sa, sbt, want


E8M0_K = 8192  # 256 blocks: row i's one element sits in block i


def e8m0_range_case():
    """FP8, every scale byte 1 .. 254 on the A side: ``A[i][32 i]`` is 1.0 (code 0x38), the rest of
    the row 0x00, and Bt is 1.0 throughout.  The scale of block b is ``min(max(b, 1), 254)`` in
    every row of A, so row i's element is scaled by byte i (rows 0 and 255 reuse 1 and 254);
    ``sBt[j][b]`` is ``254 - sA[b] + ((j mod 41) - 20)`` kept inside 1 .. 254.  The two exponents
    of a block then sum to -20 .. 20 in *every* block, also where A is zero, so no partial
    product leaves fp32's range however the hardware forms it.  ``want[i][j]`` is the power of
    two ``2^(sA[i][i] + sBt[j][i] - 254)``."""
    m, n, k = ALL_CODES_M, ALL_CODES_N, E8M0_K
    i, j, b = np.arange(m), np.arange(n), np.arange(k // 32)
    a = np.zeros((m, k), dtype=np.uint8)
    a[i, 32 * i] = 0x38
    bt = np.full((n, k), 0x38, dtype=np.uint8)
    sblock = np.clip(b, 1, 254)
    sa = np.repeat(sblock[None, :], m, axis=0).astype(np.uint8)
    sbt = np.clip(254 - sblock[None, :] + (j[:, None] % 41 - 20), 1, 254).astype(np.uint8)
    e = sa[i, i].astype(np.int64)[:, None] + sbt[:, i].astype(np.int64).T - 254  # [i][j]
    assert e.min() >= -20 and e.max() <= 20
    return a, bt, sa, sbt, 2.0 ** e.astype(np.float64)
