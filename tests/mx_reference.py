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
