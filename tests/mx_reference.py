"""Host model of the block-scaled probe kernels (``ops/csrc/gpu_probe_mx.h``) in all five operand
formats, in numpy.

Written from the formats' definitions and the formulas the probe states, not by calling the
library.  Each format is a row of :data:`FORMATS`: a sign bit, exponent bits, mantissa bits and a
bias, decoded by one function; what its all-ones exponent means; and how its codes are packed
into the bytes of a row:

* FP8 is OCP ``e4m3fn`` (bias 7): only ``S.1111.111`` (0x7f, 0xff) is NaN, there is no infinity.
* BF8 is OCP ``e5m2`` (bias 15), with IEEE's infinities (0x7C, 0xFC) and NaNs (0x7D … 0x7F,
  0xFD … 0xFF).  Both are one byte per element.
* FP4 is ``e2m1`` (bias 1), two elements per byte, the even k in the low nibble.
* FP6 is ``e2m3`` (bias 1, subnormals m/8, largest 7.5) and BF6 ``e3m2`` (bias 3, subnormals
  m/4 · 2^-2, largest 28).  Both are packed: element k of a row is bits ``[6k, 6k + 6)`` of the row
  read as a little-endian bit string, so four elements are three bytes, a block of 32 is 24
  bytes and a row ``3K/4`` bytes.  FP4, FP6 and BF6 have neither an infinity nor a NaN.

The rest is shared: the E8M0 scale (one byte per 32 consecutive k of a row), the probe's operand
and scale families and their 15 × 21 table of expected values.  Everything is integer arithmetic
or float64 on dyadic numbers far inside 53 bits, so the GPU tests compare bit-exactly.
"""

import collections

import numpy as np

FP8, BF8, FP6, BF6, FP4 = 0, 1, 2, 3, 4  # the hardware's format codes
NAMES = {"fp8": FP8, "fp4": FP4, "bf8": BF8, "fp6": FP6, "bf6": BF6}
ROWS, COLS = 15, 21

# special: what the all-ones exponent holds ("nan": NaN at the all-ones mantissa only; "ieee": inf
# at mantissa 0, NaN elsewhere; None: ordinary numbers).  packing: "byte", "nibble" or "6bit".
Format = collections.namedtuple("Format", "ebits mbits bias special packing")
FORMATS = {
    FP8: Format(4, 3, 7, "nan", "byte"),
    BF8: Format(5, 2, 15, "ieee", "byte"),
    FP6: Format(2, 3, 1, None, "6bit"),
    BF6: Format(3, 2, 3, None, "6bit"),
    FP4: Format(2, 1, 1, None, "nibble"),
}
PACKED = (FP6, BF6)

FP4_VALUES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=np.float64)


def code_bits(fmt):
    f = FORMATS[fmt]
    return 1 + f.ebits + f.mbits


def decode_codes(fmt, codes):
    """The values of codes of ``fmt``, one code per array element (not packed): sign-magnitude,
    subnormals ``m / 2^mbits · 2^(1 - bias)``, normals ``(1 + m / 2^mbits) · 2^(e - bias)``."""
    f = FORMATS[fmt]
    c = np.asarray(codes).astype(np.int64)
    assert ((c >= 0) & (c < 1 << code_bits(fmt))).all()
    emax, mmax = (1 << f.ebits) - 1, (1 << f.mbits) - 1
    e, m = (c >> f.mbits) & emax, c & mmax
    frac = m / float(1 << f.mbits)
    mag = np.where(e == 0, frac * 2.0 ** (1 - f.bias), (1 + frac) * 2.0 ** (e - f.bias).astype(np.float64))
    if f.special == "nan":
        mag = np.where((e == emax) & (m == mmax), np.nan, mag)
    elif f.special == "ieee":
        mag = np.where(e == emax, np.where(m == 0, np.inf, np.nan), mag)
    return np.where(c >> (f.ebits + f.mbits), -mag, mag)


def code_values(fmt):
    """The value of every code of the format, by code."""
    return decode_codes(fmt, np.arange(1 << code_bits(fmt)))


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
    """Element k of ``row`` of a packed 6-bit array becomes ``code``, in place; its neighbours keep theirs."""
    assert 0 <= code < 64
    bit = 6 * k
    for b in range(bit // 8, (bit + 5) // 8 + 1):  # the one or two bytes the element touches
        lo = max(bit, 8 * b) - 8 * b
        hi = min(bit + 6, 8 * b + 8) - 8 * b
        mask = ((1 << (hi - lo)) - 1) << lo
        part = ((code >> (max(bit, 8 * b) - bit)) << lo) & mask
        packed[row, b] = (int(packed[row, b]) & ~mask & 0xFF) | part


def pack(fmt, codes):
    """``[..., K]`` codes → the bytes of the public layout."""
    packing = FORMATS[fmt].packing
    if packing == "6bit":
        return pack6(codes)
    c = np.asarray(codes).astype(np.uint8)
    # two per byte: element 2b in the low nibble of byte b, element 2b + 1 in the high
    return (c[..., 0::2] | (c[..., 1::2] << 4)).astype(np.uint8) if packing == "nibble" else c


def unpack(fmt, packed):
    """The bytes of the public layout → ``[..., K]`` codes."""
    packing = FORMATS[fmt].packing
    if packing == "6bit":
        return unpack6(packed)
    p = np.asarray(packed, dtype=np.uint8)
    if packing == "nibble":
        return np.stack([p & 15, p >> 4], axis=-1).reshape(*p.shape[:-1], p.shape[-1] * 2)
    return p


def decode(fmt, packed):
    """The values of an operand in the public layout ([rows, row bytes] → [rows, K])."""
    return decode_codes(fmt, unpack(fmt, packed))


def encode(fmt, values):
    """Codes of exactly representable ``values`` ([rows, K]) in the public layout; 0 is +0."""
    lut = {}
    for c, x in enumerate(code_values(fmt)):
        if x == x and not (x == 0 and c != 0):
            lut[float(x)] = c
    codes = np.vectorize(lambda x: lut[float(x)], otypes=[np.uint8])(np.asarray(values, dtype=np.float64))
    return pack(fmt, codes)


def scale_values(scales):
    """E8M0 bytes → 2^(byte - 127)."""
    return 2.0 ** (np.asarray(scales, dtype=np.int64) - 127).astype(np.float64)


def scaled(fmt, codes, scales):
    """The operand a block-scaled GEMM multiplies: decoded values times their block's scale."""
    return decode(fmt, codes) * np.repeat(scale_values(scales), 32, axis=-1)


def product(fmt, a, bt, sa, sbt):
    with np.errstate(invalid="ignore"):  # inf · 0 and inf - inf are NaN, as IEEE says
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
# product of the decoded, scaled operands) must agree, which ``test_probe_mx.py`` and
# ``test_probe_mx_formats.py`` check.

ALL_CODES_M = ALL_CODES_N = 256
SCALE_LO, SCALE_HI = 119, 135  # seeded scales of the one-hot cases: 2^-8 .. 2^8


def all_codes_case(fmt):
    """Every code of ``fmt`` against every code, 256 × 256 at one stage (K = 64 for FP8 and BF8,
    128 for the others), as one-hot rows.

    Row i of A holds its code at ``k = i % K`` and code 0 elsewhere, and ``Bt[j]`` is code
    ``j % codes`` throughout.  Row i's code is ``i`` (FP8, BF8), ``i % 16`` (FP4: -0, code 8,
    included) or ``(i + 21 (i >> 7)) % 64`` (FP6, BF6: all 64 codes, -0 = 0x20 included, at all 128
    positions of a stage and so all four bit offsets of the packing, two codes per position).
    Scales are seeded per row and block in 119 .. 135.  Returns ``a, bt, sa, sbt, want``;
    ``want[i][j]`` is the IEEE product ``decode(i) · decode(j) · 2^(sA + sBt - 254)`` of the block
    that holds row i's element: NaN for a NaN code and for inf · 0, the same-signed infinity for
    inf · x."""
    m, n = ALL_CODES_M, ALL_CODES_N
    i, j = np.arange(m), np.arange(n)
    rng = np.random.default_rng(20240 + fmt)
    ncodes = 1 << code_bits(fmt)
    k = 64 if FORMATS[fmt].packing == "byte" else 128
    hot = i % k
    ca = (i + 21 * (i >> 7)) % 64 if fmt in PACKED else i % ncodes
    cb = j % ncodes
    codes = np.zeros((m, k), dtype=np.uint8)
    codes[i, hot] = ca
    a = pack(fmt, codes)
    bt = pack(fmt, np.repeat(cb.astype(np.uint8)[:, None], k, axis=1))
    da, db = decode_codes(fmt, ca), decode_codes(fmt, cb)
    sa = rng.integers(SCALE_LO, SCALE_HI + 1, size=(m, k // 32), dtype=np.uint8)
    sbt = rng.integers(SCALE_LO, SCALE_HI + 1, size=(n, k // 32), dtype=np.uint8)
    blk = hot // 32
    e = sa[i, blk].astype(np.int64)[:, None] + sbt[:, blk].astype(np.int64).T - 254  # [i][j]
    with np.errstate(invalid="ignore"):
        want = da[:, None] * db[None, :] * 2.0 ** e.astype(np.float64)
        # the zeros of the other k are multiplied too: a row of A whose code is finite meets Bt's
        # code j at every k, so an infinite or NaN Bt code (FP8, BF8) makes the whole column NaN
        # (0 · inf), and a NaN or infinite A code meets only its own k
        want = np.where(np.isfinite(db)[None, :], want, np.nan)
    return a, bt, sa, sbt, want


E8M0_K = 8192  # 256 blocks: row i's one element sits in block i


def e8m0_range_case(fmt=FP8):
    """Every scale byte 1 .. 254 on the A side, as FP8 or as FP6 (through the 6-bit kernel's own
    scale path): ``A[i][32 i]`` is 1.0 (code 0x38, or 0x08), the rest of the row zero, and Bt is 1.0
    throughout.  The scale of block b is ``min(max(b, 1), 254)`` in
    every row of A, so row i's element is scaled by byte i (rows 0 and 255 reuse 1 and 254);
    ``sBt[j][b]`` is ``254 - sA[b] + ((j mod 41) - 20)`` kept inside 1 .. 254.  The two exponents
    of a block then sum to -20 .. 20 in *every* block, also where A is zero, so no partial
    product leaves fp32's range however the hardware forms it.  ``want[i][j]`` is the power of
    two ``2^(sA[i][i] + sBt[j][i] - 254)``."""
    m, n, k = ALL_CODES_M, ALL_CODES_N, E8M0_K
    i, j, b = np.arange(m), np.arange(n), np.arange(k // 32)
    one = int(np.flatnonzero(code_values(fmt) == 1.0)[0])
    a = np.zeros((m, k), dtype=np.uint8)
    a[i, 32 * i] = one
    bt = np.full((n, k), one, dtype=np.uint8)
    sblock = np.clip(b, 1, 254)
    sa = np.repeat(sblock[None, :], m, axis=0).astype(np.uint8)
    sbt = np.clip(254 - sblock[None, :] + (j[:, None] % 41 - 20), 1, 254).astype(np.uint8)
    e = sa[i, i].astype(np.int64)[:, None] + sbt[:, i].astype(np.int64).T - 254  # [i][j]
    assert e.min() >= -20 and e.max() <= 20
    return pack(fmt, a), pack(fmt, bt), sa, sbt, 2.0 ** e.astype(np.float64)
