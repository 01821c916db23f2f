"""Host model of the probe's FP32 / FP64 kernels (``ops/csrc/gpu_probe_fp.h``), in numpy.

Written from the formulas the kernel comments state, not by calling the library: the probe's
operand families times odd constants, their 5 × 7 closed form, the bound under which every
partial sum is an exact integer of the accumulator type, and a one-hot case in which every output
is a single rounded product.
"""

import numpy as np

import probe_reference as ref

FORMATS = ["f32", "f64"]
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
NP_BITS = {"f32": np.int32, "f64": np.int64}
STAGE = {"f32": 16, "f64": 8}  # elements per 64-byte stage of a row
TILE_N = {"f32": 256, "f64": 128}  # columns of a workgroup tile (rows: 256)
MUL = {"f32": (25, 41), "f64": (1048573, 1048575)}
EXACT_BELOW = {"f32": 2 ** 24, "f64": 2 ** 53}  # integers the accumulator type holds exactly
MANTISSA = {"f32": 23, "f64": 52}
EXP_BIAS = {"f32": 127, "f64": 1023}


def k_exact(fmt, k):
    """Every partial sum of the probe operands is at most ``6 K MUL_A MUL_B`` in magnitude
    (``|a| <= 2 MUL_A``, ``|b| <= 3 MUL_B``): exact in any summation order below ``EXACT_BELOW``."""
    return 6 * k * MUL[fmt][0] * MUL[fmt][1] < EXACT_BELOW[fmt]


def operand_values(fmt, m, n, k):
    """The operands ``fp_fill_kernel`` writes, as int64."""
    a, bt = ref.probe_operands(m, n, k)
    return a * MUL[fmt][0], bt * MUL[fmt][1]


def operands(fmt, m, n, k):
    """The same in the format's own type."""
    a, bt = operand_values(fmt, m, n, k)
    return a.astype(NP_DTYPE[fmt]), bt.astype(NP_DTYPE[fmt])


def table(fmt, k):
    """Expected ``C[i][j]`` by ``(i mod 5, j mod 7)`` as int64: the bf16 probe's table times
    ``MUL_A MUL_B``."""
    return ref.probe_class_table(k) * (MUL[fmt][0] * MUL[fmt][1])


def expected(fmt, m, n, k):
    return table(fmt, k)[np.arange(m)[:, None] % 5, np.arange(n)[None, :] % 7]


def tiles(fmt, m, n):
    return (m // 256) * (n // TILE_N[fmt])


def sweep_values(fmt, v, side):
    """The integers of A (``side`` 0) or Bt (1) with element ``x mod K`` of every row x one step of the
    family, ``MUL_A`` resp. ``MUL_B``, higher: at most ``3 MUL_A`` resp. ``4 MUL_B`` in magnitude."""
    out = np.array(v, dtype=np.int64)
    idx = np.arange(out.shape[0])
    out[idx, idx % out.shape[1]] += MUL[fmt][side]
    return out


# ------------------------------------------------------------------ value against value


def values(fmt, seed):
    """256 normal numbers of the format as bit patterns (int32 / int64), seeded: mantissas all
    ones (every fourth), a single bit (every fourth: each bit position in turn), and random full
    ones; random signs; unbiased exponents spread over ±63 (f32) resp. ±511 (f64), both ends
    included, so that every product of two of them is a normal number."""
    mb, bias = MANTISSA[fmt], EXP_BIAS[fmt]
    span = 63 if fmt == "f32" else 511
    rng = np.random.default_rng(seed)
    i = np.arange(256)
    exp = rng.integers(-span, span + 1, size=256)
    exp[:4] = [-span, span, -span, span]
    mant = rng.integers(0, 2 ** mb, size=256, dtype=np.int64)
    mant[i % 4 == 0] = 2 ** mb - 1
    single = i % 4 == 1
    mant[single] = 1 << ((i[single] // 4) % mb)
    sign = rng.integers(0, 2, size=256, dtype=np.int64)
    ebits = 8 if fmt == "f32" else 11
    bits = (sign << (mb + ebits)) | ((exp + bias).astype(np.int64) << mb) | mant  # f64: the sign wraps into bit 63
    return bits.astype(np.uint32).view(np.int32) if fmt == "f32" else bits


def onehot_case(fmt):
    """256 values against 256 others at one stage: ``A[i][k]`` is value ``i`` of the first set at
    ``k = i % stage`` and +0 elsewhere, ``Bt[j][k]`` is value ``j`` of the second set at every k.
    Each output is one product, rounded once to nearest even (``np.float32(a) * np.float32(b)``
    resp. the float64 product), plus exact zeros.  Returns ``a, bt, want`` in the format's type."""
    dt, stage = NP_DTYPE[fmt], STAGE[fmt]
    va = values(fmt, 320032 if fmt == "f32" else 640064).view(dt)
    vb = values(fmt, 320033 if fmt == "f32" else 640065).view(dt)
    i = np.arange(256)
    a = np.zeros((256, stage), dtype=dt)
    a[i, i % stage] = va
    bt = np.repeat(vb[:, None], stage, axis=1)
    want = va[:, None] * vb[None, :]
    assert want.dtype == dt
    return a, bt, want
