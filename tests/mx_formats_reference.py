"""Host model of the BF8 / FP6 / BF6 block-scaled probe kernels (``ops/csrc/gpu_probe_mx.h``), in numpy.

Written from the formats' definitions, as ``mx_reference.py`` is for FP8 and FP4, whose shared
pieces (the E8M0 scale, the probe's operand and scale families and their 15 × 21 table) it
imports:

* BF8 is OCP ``e5m2``: 1 sign, 5 exponent (bias 15), 2 mantissa bits, with IEEE's infinities
  (0x7C, 0xFC) and NaNs (0x7D … 0x7F, 0xFD … 0xFF); one byte per element.
* FP6 is ``e2m3`` (bias 1, subnormals m/8, largest 7.5) and BF6 ``e3m2`` (bias 3, subnormals
  m/4 · 2^-2, largest 28); neither has an infinity or a NaN.  Both are packed: element k of a
  row is bits ``[6k, 6k + 6)`` of the row read as a little-endian bit string, so four elements
  are three bytes, a block of 32 is 24 bytes and a row ``3K/4`` bytes.

Everything is integer arithmetic or float64 on dyadic numbers far inside 53 bits, so the GPU
tests compare bit-exactly.
"""

import numpy as np

from mx_reference import probe_scales, probe_table, probe_values, scale_values  # noqa: F401  (shared pieces)
from mx_reference import ALL_CODES_M, ALL_CODES_N, E8M0_K, SCALE_HI, SCALE_LO

BF8, FP6, BF6 = 1, 2, 3  # the hardware's format codes
NAMES = {"bf8": BF8, "fp6": FP6, "bf6": BF6}
PACKED = (FP6, BF6)


def decode_bf8(codes):
    """OCP e5m2: bias 15; exponent 31 is ±inf (mantissa 0) or NaN."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 2) & 31, c & 3
    mag = np.where(e == 0, m / 4.0 * 2.0 ** -14, (1 + m / 4.0) * 2.0 ** (e - 15).astype(np.float64))
    mag = np.where(e == 31, np.where(m == 0, np.inf, np.nan), mag)
    return np.where(c & 0x80, -mag, mag)


def decode_fp6(codes):
    """e2m3 codes 0 … 63 (one per array element, not packed): bias 1, subnormals m/8."""
    c = np.asarray(codes).astype(np.int64)
    assert ((c >= 0) & (c < 64)).all()
    e, m = (c >> 3) & 3, c & 7
    mag = np.where(e == 0, m / 8.0, (1 + m / 8.0) * 2.0 ** (e - 1).astype(np.float64))
    return np.where(c & 0x20, -mag, mag)


def decode_bf6(codes):
    """e3m2 codes 0 … 63 (one per array element, not packed): bias 3, subnormals m/4 · 2^-2."""
    c = np.asarray(codes).astype(np.int64)
    assert ((c >= 0) & (c < 64)).all()
    e, m = (c >> 2) & 7, c & 3
    mag = np.where(e == 0, m / 4.0 * 2.0 ** -2, (1 + m / 4.0) * 2.0 ** (e - 3).astype(np.float64))
    return np.where(c & 0x20, -mag, mag)


def pack6(codes):
    """``[..., K]`` 6-bit codes → ``[..., 3K/4]`` bytes: element k in bits ``[6k, 6k + 6)`` of the row."""
    c = np.asarray(codes).astype(np.uint32)
    assert c.shape[-1] % 4 == 0 and (c < 64).all()
    q = c.reshape(*c.shape[:-1], -1, 4)
    w = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)  # 24 bits per four elements
    out = np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], axis=-1).astype(np.uint8)
    return out.reshape(*c.shape[:-1], -1)


def unpack6(packed):
    """``[..., 3K/4]`` bytes → ``[..., K]`` 6-bit codes, bit by bit from the layout's definition."""
    p = np.asarray(packed, dtype=np.uint8)
    bits = np.unpackbits(p, axis=-1, bitorder="little")  # bit b of the row's little-endian bit string
    six = bits.reshape(*p.shape[:-1], -1, 6).astype(np.int64)
    return (six << np.arange(6)).sum(axis=-1)


def set_code(packed, row, k, code):
    """Element k of ``row`` of a packed array becomes ``code``, in place; its neighbours keep theirs."""
    assert 0 <= code < 64
    bit = 6 * k
    for b in range(bit // 8, (bit + 5) // 8 + 1):  # the one or two bytes the element touches
        lo = max(bit, 8 * b) - 8 * b
        hi = min(bit + 6, 8 * b + 8) - 8 * b
        mask = ((1 << (hi - lo)) - 1) << lo
        part = ((code >> (max(bit, 8 * b) - bit)) << lo) & mask
        packed[row, b] = (int(packed[row, b]) & ~mask & 0xFF) | part


def decode(fmt, codes):
    """The values of an operand in the public layout ([rows, row bytes] → [rows, K])."""
    if fmt == BF8:
        return decode_bf8(codes)
    return (decode_fp6 if fmt == FP6 else decode_bf6)(unpack6(codes))


def code_values(fmt):
    """The value of every code of the format, by code."""
    return decode_bf8(np.arange(256)) if fmt == BF8 else (decode_fp6 if fmt == FP6 else decode_bf6)(np.arange(64))


def encode(fmt, values):
    """Codes of exactly representable ``values`` ([rows, K]) in the public layout; 0 is +0."""
    lut = {}
    for c, x in enumerate(code_values(fmt)):
        if x == x and not (x == 0 and c != 0):
            lut[float(x)] = c
    codes = np.vectorize(lambda x: lut[float(x)], otypes=[np.uint8])(np.asarray(values, dtype=np.float64))
    return pack6(codes) if fmt in PACKED else codes


def scaled(fmt, codes, scales):
    """The operand a block-scaled GEMM multiplies: decoded values times their block's scale."""
    return decode(fmt, codes) * np.repeat(scale_values(scales), 32, axis=-1)


def product(fmt, a, bt, sa, sbt):
    with np.errstate(invalid="ignore"):  # inf · 0 and inf - inf are NaN, as IEEE says
        return scaled(fmt, a, sa) @ scaled(fmt, bt, sbt).T


# ------------------------------------------------------------------ one-hot cases of the store kernel


def all_codes_case(fmt):
    """Every code of ``fmt`` against every code, 256 × 256 at one stage, as one-hot rows: each
    output is a single product, exact whatever the order or width the hardware sums in.

    BF8 (K = 64), as the FP8 case: ``A[i][k]`` is code ``i`` at ``k = i % 64`` and 0x00 elsewhere,
    ``Bt[j]`` is code ``j`` throughout.  FP6 / BF6 (K = 128): row i holds code
    ``(i + 21 (i >> 7)) % 64`` at ``k = i % 128`` and zeros elsewhere, ``Bt[j]`` is code ``j % 64``
    throughout: all 64 codes (-0, code 0x20, included), all 128 positions of a stage and so all
    four bit offsets of the packing, two codes per position.  Scales are seeded per row and block
    in 119 … 135.  Returns ``a, bt, sa, sbt, want``; ``want[i][j]`` is the IEEE product
    ``decode(i) · decode(j) · 2^(sA + sBt - 254)`` of the block that holds row i's element: NaN for
    a NaN code and for inf · 0, the same-signed infinity for inf · x."""
    m, n = ALL_CODES_M, ALL_CODES_N
    i, j = np.arange(m), np.arange(n)
    rng = np.random.default_rng(20240 + fmt)
    if fmt == BF8:
        k = 64
        hot = i % k
        a = np.zeros((m, k), dtype=np.uint8)
        a[i, hot] = i
        bt = np.repeat(j.astype(np.uint8)[:, None], k, axis=1)
        da, db = decode_bf8(i), decode_bf8(j)
    else:
        k = 128
        hot = i % k
        ca = (i + 21 * (i >> 7)) % 64
        codes = np.zeros((m, k), dtype=np.uint8)
        codes[i, hot] = ca
        a = pack6(codes)
        bt = pack6(np.repeat((j % 64).astype(np.uint8)[:, None], k, axis=1))
        dec = decode_fp6 if fmt == FP6 else decode_bf6
        da, db = dec(ca), dec(j % 64)
    sa = rng.integers(SCALE_LO, SCALE_HI + 1, size=(m, k // 32), dtype=np.uint8)
    sbt = rng.integers(SCALE_LO, SCALE_HI + 1, size=(n, k // 32), dtype=np.uint8)
    blk = hot // 32
    e = sa[i, blk].astype(np.int64)[:, None] + sbt[:, blk].astype(np.int64).T - 254  # [i][j]
    with np.errstate(invalid="ignore"):
        want = da[:, None] * db[None, :] * 2.0 ** e.astype(np.float64)
        if fmt == BF8:
            # the zeros of the other 63 k are multiplied too: a row of A whose code is finite meets
            # Bt's code j at every k, so an infinite or NaN Bt code makes the whole column NaN
            # (0 · inf), and a NaN or infinite A code meets only its own k
            want = want + np.where(np.isfinite(db), 0.0, np.nan)[None, :]
    return a, bt, sa, sbt, want


def e8m0_range_case():
    """``mx_reference.e8m0_range_case`` re-encoded as FP6: every scale byte 1 … 254 on the A side
    through the FP6 kernel's own scale path.  ``A[i][32 i]`` is 1.0 (code 0x08), the rest of the row
    zero, Bt is 1.0 throughout, K = 8192; scales and expected powers of two as there."""
    from mx_reference import e8m0_range_case as fp8_case

    a8, bt8, sa, sbt, want = fp8_case()
    assert a8.shape[1] == E8M0_K
    a = pack6(np.where(a8 == 0x38, 0x08, 0).astype(np.uint8))
    bt = pack6(np.where(bt8 == 0x38, 0x08, 0).astype(np.uint8))
    return a, bt, sa, sbt, want
