"""What ``test_gpu_dcvt_edges.py`` stands on, checked without a GPU: the cases of ``dcvt_cases.py`` are what they
claim to be, the reference (float64 product, one cast by numpy / torch) is round-to-nearest-even done in integers at
every code and scale byte, inside the exact windows it is the integer construction the device's self-check uses, and
the comparisons report a single flipped bit at the right place."""

import numpy as np
import pytest
import torch

import dcvt_cases as dc
import mx_reference as ref
from test_gpu_dcvt import DTYPES, FORMATS, WINDOW

# a destination: mantissa bits, smallest normal exponent, exponent bits
DST = {torch.float32: (23, -126, 8), torch.float16: (10, -14, 5), torch.bfloat16: (7, -126, 8)}
IDS = ["f32", "f16", "bf16"]


def _finite_magnitudes(fmt):
    """``(code, m, e)`` of every finite positive code but zero: its value is ``m · 2^e`` with integers m > 0 and e, from
    the format's definition."""
    f = ref.FORMATS[ref.NAMES[fmt]]
    table = ref.code_values(ref.NAMES[fmt])
    out = []
    for code in range(1, 1 << (f.ebits + f.mbits)):
        if not np.isfinite(table[code]):
            continue
        ef, mf = code >> f.mbits, code & ((1 << f.mbits) - 1)
        m, e = (mf, 1 - f.bias - f.mbits) if ef == 0 else ((1 << f.mbits) | mf, ef - f.bias - f.mbits)
        assert m * 2.0 ** e == table[code]
        out.append((code, m, e))
    assert len(out) == {"fp8": 126, "bf8": 123, "fp4": 7, "fp6": 31, "bf6": 31}[fmt]
    return out


def _rne_bits(m, e, p, emin, ebits):
    """The bits, sign apart, of ``m · 2^e`` (integers, m > 0) rounded to nearest even into a binary format with ``p``
    mantissa bits, smallest normal exponent ``emin`` and ``ebits`` exponent bits, overflow to infinity.  Python integers only."""
    x = m.bit_length() - 1 + e  # the value lies in [2^x, 2^(x + 1))
    q = max(x, emin) - p  # the weight of the last kept bit; subnormals share emin's
    if e >= q:
        n = m << (e - q)
    else:
        n, rem, half = m >> (q - e), m & ((1 << (q - e)) - 1), 1 << (q - e - 1)
        n += rem > half or (rem == half and n & 1)
    # n counts units of 2^q: below 2^p a subnormal (or zero), from 2^p on the hidden bit adds one to the field; a
    # carry out of the mantissa moves into the exponent field by itself
    bits = n + ((max(x, emin) - emin) << p)
    return min(bits, ((1 << ebits) - 1) << p)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_pair_case_is_what_it_says(fmt):
    codes, scales, values = dc.every_pair_case(fmt)  # asserts completeness, neighbours and the NaN count itself
    k, nrot = dc.EVERY_PAIR[fmt]
    from odh_kubeflow_amd.ops import gpu

    assert codes.dtype == scales.dtype == np.uint8 and values.dtype == np.float64
    assert codes.shape == (256 * nrot, gpu.mx_row_bytes(fmt, k)) and scales.shape == (256 * nrot, k // 32)
    assert values.shape == (256 * nrot, k) and values.size <= 2048 * 256
    # the values by another route: the packed bytes decoded by the model of the layout
    byte = np.repeat(scales.astype(np.int64), 32, axis=1)
    want = np.where(byte == 255, np.nan, ref.scaled(ref.NAMES[fmt], codes, scales))
    assert np.array_equal(values, want, equal_nan=True)
    assert np.isnan(values[byte == 255]).all() and (values == 0).any() and np.signbit(values[values == 0]).any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_cap_pattern_is_what_it_says(fmt):
    codes, scales, values = dc.cap_pattern(fmt)  # asserts the scale bytes, the zero blocks and bf8's infinities itself
    from odh_kubeflow_amd.ops import gpu

    assert codes.shape == (1 << 15, gpu.mx_row_bytes(fmt, 32)) and scales.shape == (1 << 15, 1) and values.shape == (1 << 15, 32)
    assert not np.isnan(values).any() and scales.max() == 254 and scales.min() == 0
    assert not codes[::16].any() and codes[1::16].any()
    assert np.array_equal(values, ref.scaled(ref.NAMES[fmt], codes, scales))
    for dtype in DTYPES:  # determined bits: nothing is compared by class
        assert not dc.expected_bits(values, dtype)[1].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_is_round_to_nearest_even_in_integers(fmt, dtype):
    """Every finite non-zero code, both signs, at every scale byte 0 … 254: subnormal results, ties, overflow."""
    p, emin, ebits = DST[dtype]
    f = ref.FORMATS[ref.NAMES[fmt]]
    sign_code, sign_bit = 1 << (f.ebits + f.mbits), 1 << (p + ebits)
    mags = _finite_magnitudes(fmt)
    byte = np.arange(255)
    want = np.array([[_rne_bits(m, e + int(b) - 127, p, emin, ebits) for b in byte] for _, m, e in mags], dtype=np.int64)
    inf = ((1 << ebits) - 1) << p
    assert inf == dc.INF[dtype] and (want <= inf).all()
    assert ((want > 0) & (want < 1 << p)).any() and (want == inf).any()  # the classes the windows leave out
    # rounded away altogether: below half of 2^-24 in float16, and fp8's 2^-136 and bf8's 2^-143 below half of bfloat16's
    # 2^-133; float32's 2^-149 holds every product
    assert (want == 0).any() == (dtype == torch.float16 or (dtype == torch.bfloat16 and fmt in ("fp8", "bf8")))
    for s in (0, 1):
        code = np.array([c for c, _, _ in mags]) | s * sign_code
        got, nan = dc.expected_bits(dc.scaled_values(fmt, code[:, None], byte[None, :]), dtype)
        assert not nan.any()
        assert np.array_equal(got & (2 * sign_bit - 1), want | s * sign_bit)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_is_the_device_construction_inside_the_window(fmt, dtype):
    """``sign | (bias + p + e + byte - 127) << mbits | mantissa``: what ``dcvt_expect`` builds for the fused check."""
    window = WINDOW[fmt, 16 if dtype == torch.float16 else 32]
    if window is None:
        assert (fmt, dtype) == ("bf8", torch.float16)
        return
    mb, emin, ebits = DST[dtype]
    bias, sb = 1 - emin, mb + ebits
    f = ref.FORMATS[ref.NAMES[fmt]]
    sign_code = 1 << (f.ebits + f.mbits)
    byte = np.arange(window[0], window[1] + 1)
    codes, want = [0, sign_code], [[0] * len(byte), [1 << sb] * len(byte)]
    for code, m, e in _finite_magnitudes(fmt):
        p = m.bit_length() - 1
        row = [(bias + p + e + int(b) - 127) << mb | (m << (mb - p)) & ((1 << mb) - 1) for b in byte]
        assert 1 << mb <= min(row) and max(row) < dc.INF[dtype]  # normal and finite: the window is exact
        codes += [code, code | sign_code]
        want += [row, [1 << sb | r for r in row]]
    got, nan = dc.expected_bits(dc.scaled_values(fmt, np.array(codes)[:, None], byte[None, :]), dtype)
    assert not nan.any() and np.array_equal(got & ((2 << sb) - 1), np.array(want, dtype=np.int64))
    # and one byte further out the construction no longer holds for the smallest or the largest code
    lo, hi = window
    below = dc.expected_bits(dc.scaled_values(fmt, [1], [lo - 1]), dtype)[0][0]
    cmax = max(c for c, _, _ in _finite_magnitudes(fmt))
    above = dc.expected_bits(dc.scaled_values(fmt, [cmax], [hi + 1]), dtype)[0][0]
    assert 0 < below < 1 << mb and above == dc.INF[dtype]


# ------------------------------------------------------------------ the comparisons can fail, and say where


def _as_tensor_bits(values, dtype):
    bits, _ = dc.expected_bits(values, dtype)
    return bits.copy()


def test_a_flipped_bit_of_a_subnormal_float16_is_reported_by_its_triple():
    codes, scales, values = dc.every_pair_case("fp8")
    got = _as_tensor_bits(values, torch.float16)
    dc.assert_equals_reference("clean", got, values, torch.float16, dc.triple_of("fp8", codes, scales))
    sub = np.flatnonzero((((got & 0x7C00) == 0) & ((got & 0x3FF) != 0)).ravel())
    assert sub.size > 1000
    i = int(sub[sub.size // 2])
    row, j = divmod(i, 256)
    want = int(got.ravel()[i])
    got.ravel()[i] ^= 1
    with pytest.raises(pytest.fail.Exception) as e:
        dc.assert_equals_reference("fp8 f16", got, values, torch.float16, dc.triple_of("fp8", codes, scales))
    text = str(e.value)
    assert "1 of 524288 elements differ" in text, text
    assert f"(code 0x{codes[row, j]:02x}, scale byte {scales[row, j // 32]}, position {j % 8})" in text, text
    assert f"got 0x{want ^ 1:04x} want 0x{want:04x}" in text, text


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_minus_zero_that_lost_its_sign_is_reported(dtype):
    codes, scales, values = dc.every_pair_case("fp4")
    got = _as_tensor_bits(values, dtype)
    sign = -(1 << 15) if dtype != torch.float32 else -(1 << 31)  # as the signed integers of the view
    zeros = np.flatnonzero((got.ravel() == sign) & (values.ravel() == 0))  # the code -0, not a product rounded to it
    assert zeros.size and np.signbit(values.ravel()[zeros]).all()
    i = int(zeros[-1])
    got.ravel()[i] = 0  # +0: equal by value, not by bits
    with pytest.raises(pytest.fail.Exception) as e:
        dc.assert_equals_reference("fp4", got, values, dtype, dc.triple_of("fp4", codes, scales))
    row, j = divmod(i, 64)
    digits = 8 if dtype == torch.float32 else 4
    assert "1 of " in str(e.value) and f"(code 0x08, scale byte {scales[row, j // 32]}, position {j % 8})" in str(e.value)
    assert f"got 0x{0:0{digits}x} want 0x{8 << 4 * (digits - 1):0{digits}x}" in str(e.value), str(e.value)


def test_a_nan_is_compared_by_class_and_an_infinity_in_its_place_is_reported():
    codes, scales, values = dc.every_pair_case("bf8")
    got = _as_tensor_bits(values, torch.float32)
    nan = np.flatnonzero(np.isnan(values).ravel())
    got.ravel()[nan] = 0x7FC00001  # another NaN than the cast's: still right
    dc.assert_equals_reference("bf8", got, values, torch.float32)
    got.ravel()[nan[5]] = 0x7F800000
    with pytest.raises(pytest.fail.Exception, match=r"1 of 524288 elements differ: element %d got 0x7f800000 want a NaN" % nan[5]):
        dc.assert_equals_reference("bf8", got, values, torch.float32)


def test_a_flipped_bit_in_the_last_slab_beyond_the_cap_is_reported():
    rows = 524289
    _, _, values = dc.cap_pattern("fp8")
    want = dc.tiled(torch.from_numpy(dc.expected_bits(values, torch.float32)[0].astype(np.int32)), rows)
    assert tuple(want.shape) == (rows, 32) and rows * 32 // 4 == 4096 * 1024 + 8  # the last slab: 8 pieces, one block
    got = want.clone()
    dc.assert_blocks_equal("clean", got, want)
    got[rows - 1, 31] ^= 1 << 22
    with pytest.raises(pytest.fail.Exception, match=r"1 of 524289 blocks differ, the first at \[524288\], the last at 524288"):
        dc.assert_blocks_equal("fp8 f32", got, want)
    got[1 << 15, 0] ^= 1  # and the first block of the second tile
    with pytest.raises(pytest.fail.Exception, match=r"2 of 524289 blocks differ, the first at \[32768, 524288\], the last at 524288"):
        dc.assert_blocks_equal("fp8 f32", got, want)


def test_a_written_guard_byte_is_reported_on_either_side():
    nbytes = 4112
    buf = torch.full((dc.GUARD + nbytes + dc.GUARD,), dc.GUARD_FILL, dtype=torch.uint8)
    buf[dc.GUARD:dc.GUARD + nbytes] = 0
    dc.assert_guards_untouched("clean", buf, nbytes)
    for at in (dc.GUARD + nbytes, dc.GUARD - 1, 0, len(buf) - 1):
        buf[at] ^= 1
        with pytest.raises(pytest.fail.Exception, match=r"1 bytes written outside out\[0:4112\], at offsets \[%d\]" % (at - dc.GUARD)):
            dc.assert_guards_untouched("guard", buf, nbytes)
        buf[at] ^= 1
