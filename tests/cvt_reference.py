"""Host model of the converter kernels (``ops/csrc/gpu_probe_cvt.h``), in numpy.

Written from the formats' definitions (``mx_reference.FORMATS``) and the rules the probe states, not by
calling the library:

* :func:`encode` — what a scaled converter returns for any f32 and any E8M0 scale byte: the exact quotient
  ``x / 2^(byte - 127)`` (float64 holds it: an f32 has 24 significant bits and the exponents stay far inside
  float64's) rounded to nearest even on the format's grid, subnormals included, and the recorded answer of
  the hardware for what lies at or beyond half a step above the largest finite value (:data:`OVERFLOW`);
  bf16 by integer arithmetic on the bits.
* :func:`family` — the input family of the fused check with its expected codes *by construction*: no
  rounding happens in it.  :func:`encode` applied to its inputs must give its expectations.
* :func:`quantize` — the public operation: OCP MX scales and saturating codes, in the layout ``mx_gemm`` reads.

The contract of the public operation for every f32, non-finite ones included (the same words as in
``gpu_probe_cvt.h`` and ``gpu.mx_quantize``).  For the scaled formats, per block of 32:

* amax is the largest ``|x|`` over the elements that are not NaN; ±Inf counts as FLT_MAX.
* If no such element exists, or all are zero, the scale byte is 127.
* Otherwise the byte is ``clamp(floor(log2 amax) - emax + 127, 0, 254)``; with an Inf in the block that is
  ``254 - emax``.  Byte 255 is never emitted.
* Finite elements are clamped in f32 to ±(largest finite value · scale) and then converted.
* ±Inf becomes the largest finite code with its sign, in every format: the saturation of finite overflow.
* NaN goes to the instruction unclamped and becomes what :data:`NAN_CODE` records: fp8 0xFF and bf8 0xFE
  whatever the sign; fp4, fp6 and bf6 have no NaN and give their largest code with the input's sign, so these
  three formats cannot carry a NaN.

bf16 is the plain conversion: Inf stays Inf, NaN stays NaN, quieted.
"""

import numpy as np

import mx_reference as mx

FP8, BF8, FP6, BF6, FP4, BF16 = 0, 1, 2, 3, 4, 5
NAMES = {"fp8": FP8, "bf8": BF8, "fp4": FP4, "fp6": FP6, "bf6": BF6, "bf16": BF16}  # the order of --cvt
SCALED = (FP8, BF8, FP6, BF6, FP4)
CMAX = {FP8: 126, BF8: 123, FP4: 7, FP6: 31, BF6: 31}  # the largest finite magnitude code
NSEL = {FP8: 2, BF8: 2, FP4: 4, FP6: 1, BF6: 1}  # destination selects of the instruction
# (code at exactly half a step above the largest finite value, code beyond it), as recorded from the hardware:
# e4m3fn rounds the tie to its even largest code and gives NaN beyond it, e5m2 gives infinity from the tie on
# (its largest code is odd), and the formats that have neither saturate
OVERFLOW = {FP8: (126, 0x7F), BF8: (0x7C, 0x7C), FP4: (7, 7), FP6: (31, 31), BF6: (31, 31)}
# of a NaN input (outside the probe's family), whatever its sign; the other formats give their largest code
# with the input's sign
NAN_CODE = {FP8: 0xFF, BF8: 0xFE}
# of any input, zero included, at scale byte 255 (the E8M0 NaN), as recorded from the hardware: what a NaN
# input gives.  The format's NaN whatever the input's sign, or the largest code with the input's sign (the
# magnitude code here; an earlier single measurement had taken it for the positive code).  The quantiser
# never emits that byte
SCALE_NAN_CODE = {FP8: 0xFF, BF8: 0xFE, FP4: 7, FP6: 31, BF6: 31}
FLT_MAX = float(np.finfo(np.float32).max)
BF16_EXPS = 254


def sign_bit(fmt):
    return 15 if fmt == BF16 else mx.code_bits(fmt) - 1


def magnitudes(fmt):
    """v(c) for c = 0 … cmax."""
    return mx.code_values(fmt)[:CMAX[fmt] + 1]


def emax(fmt):
    """Exponent of the largest finite value."""
    return int(np.floor(np.log2(magnitudes(fmt)[-1])))


def overflow_midpoint(fmt):
    """Half a step above the largest finite value."""
    v = magnitudes(fmt)
    return v[-1] + (v[-1] - v[-2]) / 2


def encode(fmt, x, scale_bytes=127):
    """Codes (one per element, sign included, not packed) of f32 ``x`` divided by ``2^(scale_bytes - 127)``;
    at scale byte 255 :data:`SCALE_NAN_CODE`, with the input's sign where the format has no NaN."""
    x = np.asarray(x, dtype=np.float32)
    if fmt == BF16:
        bits = x.view(np.uint32).astype(np.uint64)
        out = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.int64)
        nan = np.isnan(x)
        return np.where(nan, (bits >> 16).astype(np.int64) | 0x40, out)  # a NaN stays one, quieted
    f = mx.FORMATS[fmt]
    sb = np.broadcast_to(np.asarray(scale_bytes, dtype=np.int64), x.shape)
    y = np.abs(x.astype(np.float64)) * 2.0 ** (127 - sb).astype(np.float64)
    neg = np.signbit(x)
    finite = np.isfinite(y)
    ys = np.where(finite, y, 0.0)
    _, ex = np.frexp(ys)  # ys = m · 2^ex, 0.5 <= m < 1: floor(log2) = ex - 1
    e = np.where(ys == 0, 1 - f.bias, np.maximum(ex - 1, 1 - f.bias))  # subnormals share the smallest normal's quantum
    q = 2.0 ** (e - f.mbits).astype(np.float64)
    k = np.rint(ys / q).astype(np.int64)  # nearest, ties to even: ys / q is exact
    # k in [0, 2^(mbits + 1)]: the magnitude code is the grid index; a carry into the next binade is the
    # next code by the same arithmetic
    code = np.where(e == 1 - f.bias, k, ((e + f.bias) << f.mbits) + (k - (1 << f.mbits)))
    mid = overflow_midpoint(fmt)
    tie, beyond = OVERFLOW[fmt]
    code = np.where(ys < mid, np.minimum(code, CMAX[fmt]), np.where(ys == mid, tie, beyond))
    code = np.where(np.isinf(y), beyond, code)
    code = np.where(np.isnan(y), CMAX[fmt], code) | (neg.astype(np.int64) << sign_bit(fmt))
    code = np.where(np.isnan(y), NAN_CODE[fmt], code) if fmt in NAN_CODE else code
    signed = 0 if fmt in NAN_CODE else neg.astype(np.int64) << sign_bit(fmt)
    return np.where(sb == 255, SCALE_NAN_CODE[fmt] | signed, code)


# ------------------------------------------------------------------ the family of the fused check


def scale_range(fmt):
    """The scale exponents e at which every case of the family, times 2^e, is a normal finite f32: the
    smallest input lies in the binade below the midpoint of 0 and v(1), the largest is four times the
    overflow midpoint."""
    f = mx.FORMATS[fmt]
    lo = -126 - (int(np.log2(magnitudes(fmt)[1] / 2)) - 1)
    hi = 127 - int(np.floor(np.log2(4 * overflow_midpoint(fmt))))
    assert lo == -126 + f.bias + f.mbits + 1
    return lo, hi


def variants(fmt):
    """One sign and scale of the family, unscaled: float64 values (all exact f32), a step in f32 ulps to take
    from each (-1, 0, +1), and the expected magnitude codes.  Exact codes, then (tie, below, above) per
    c < cmax, then the overflow class, then exact codes as padding to a multiple of 16."""
    cmax = CMAX[fmt]
    v = magnitudes(fmt)
    c = np.arange(cmax)
    mids = (v[:-1] + v[1:]) / 2
    vals = [v, np.repeat(mids, 3)]
    steps = [np.zeros(cmax + 1, dtype=np.int64), np.tile([0, -1, 1], cmax)]
    want = [np.arange(cmax + 1), np.stack([c + (c & 1), c, c + 1], axis=1).reshape(-1)]
    mid = overflow_midpoint(fmt)
    tie, beyond = OVERFLOW[fmt]
    vals.append(np.array([mid, mid, mid, 4 * mid]))
    steps.append(np.array([-1, 0, 1, 0]))
    want.append(np.array([cmax, tie, beyond, beyond]))
    n = sum(len(a) for a in vals)
    pad = np.arange(-n % 16) % (cmax + 1)
    vals.append(v[pad])
    steps.append(np.zeros(len(pad), dtype=np.int64))
    want.append(pad)
    return np.concatenate(vals), np.concatenate(steps), np.concatenate(want)


def family(fmt):
    """``x`` (float32), ``scale`` (E8M0 bytes; 127 for bf16), ``sel`` and ``expect`` (codes with sign) of every
    case, in the library's order: scale index, select, sign, variant."""
    if fmt == BF16:
        sign, ef, m, var = np.meshgrid(np.arange(2), np.arange(1, BF16_EXPS + 1), np.arange(128), np.arange(4),
                                       indexing="ij")
        c = (ef << 7) | m
        low = np.array([0, 0x8000, 0x7FFF, 0x8001])[var]  # exact, tie, below, above
        want = np.choose(var, [c, c + (c & 1), c, c + 1])
        bits = (sign.astype(np.uint32) << 31) | (c.astype(np.uint32) << 16) | low.astype(np.uint32)
        n = bits.size
        return {"x": bits.reshape(-1).view(np.float32), "scale": np.full(n, 127, dtype=np.uint8),
                "sel": np.zeros(n, dtype=np.uint8), "expect": (want | (sign << 15)).reshape(-1).astype(np.int64)}
    vals, steps, want = variants(fmt)
    lo, hi = scale_range(fmt)
    base = vals.astype(np.float32)
    assert (base.astype(np.float64) == vals).all()
    # one f32 ulp down or up: on the bits (the values are positive, or zero with step 0)
    stepped = (base.view(np.int32) + steps.astype(np.int32)).view(np.float32)
    e = np.arange(lo, hi + 1)
    with np.errstate(over="raise", under="raise"):
        mag = np.ldexp(stepped[None, :].astype(np.float64), e[:, None])  # exact: a power of two
    mag32 = mag.astype(np.float32)
    assert (mag32.astype(np.float64) == mag).all()
    nsel, nv = NSEL[fmt], len(vals)
    shape = (len(e), nsel, 2, nv)
    sgn = np.broadcast_to(np.arange(2)[None, None, :, None], shape)
    x = np.where(sgn == 1, -mag32[:, None, None, :], mag32[:, None, None, :]).astype(np.float32)
    expect = np.broadcast_to(want[None, None, None, :], shape) | (sgn << sign_bit(fmt))
    return {"x": x.reshape(-1), "scale": np.broadcast_to((e + 127)[:, None, None, None], shape).reshape(-1).astype(np.uint8),
            "sel": np.broadcast_to(np.arange(nsel)[None, :, None, None], shape).reshape(-1).astype(np.uint8),
            "expect": expect.reshape(-1).astype(np.int64)}


# ------------------------------------------------------------------ the public operation


def mx_scales(fmt, x):
    """OCP MX: per block of 32 along the last axis, ``floor(log2(amax)) - emax`` as an E8M0 byte clamped to
    0 … 254, amax over the elements that are not NaN with ±Inf counted as FLT_MAX; the byte of 2^0 for a block
    that is all zero or has nothing but NaN."""
    x = np.asarray(x, dtype=np.float32)
    mag = np.abs(x.astype(np.float64))
    mag = np.where(np.isnan(mag), 0.0, np.minimum(mag, FLT_MAX))
    amax = mag.reshape(*x.shape[:-1], -1, 32).max(axis=-1)
    _, ex = np.frexp(amax)
    byte = np.clip(ex - 1 - emax(fmt) + 127, 0, 254)
    return np.where(amax == 0, 127, byte).astype(np.uint8)


def quantize(fmt, x):
    """``(codes, scales)`` of f32 ``x`` ``[rows, K]``: the public layout of ``mx_gemm``; saturating, ±Inf
    included; a NaN stays one where the format has one (the module's docstring).  bf16:
    ``(uint16 bits [rows, K], None)``."""
    x = np.asarray(x, dtype=np.float32)
    if fmt == BF16:
        return encode(BF16, x).astype(np.uint16), None
    scales = mx_scales(fmt, x)
    per = np.repeat(scales.astype(np.int64), 32, axis=-1)
    lim = np.minimum(magnitudes(fmt)[-1] * 2.0 ** (per - 127).astype(np.float64), FLT_MAX)
    assert (lim.astype(np.float32).astype(np.float64) == lim).all()  # the clamp happens in f32
    clamped = np.clip(x.astype(np.float64), -lim, lim)  # np.clip keeps a NaN
    with np.errstate(invalid="ignore"):
        return mx.pack(fmt, encode(fmt, clamped.astype(np.float32), per).astype(np.uint8)), scales
