"""The converter kernels on a real MI355X against the host model (``cvt_reference.py``) at f32's edges, where
``test_gpu_cvt_exact.py`` does not go: every binade of a block's amax down to the subnormals and up to
FLT_MAX (scale bytes 0 and 254 - emax), scale bytes 0 and 255 as operands, non-finite input to ``mx_quantize``
(the contract in its docstring), bf16 of subnormals, infinities and NaN, and shapes beyond the grid cap of
4096 workgroups, where slabs grow past 1024 pieces and the trailing workgroups have nothing to do.

Everything is bit-exact.  Inputs are built as bit patterns; nothing is filtered afterwards.  The tests feed
data only: every pointer handed to a kernel comes from a torch allocation of exactly the size the shape
implies.

Beyond the cap only the 8-lane path (fp8, bf8, fp4, bf16: 16-byte pieces) is run, with fp8, fp4 and bf16.
The 6-bit path counts blocks, not pieces: its cap lies at 4096 · 1024 blocks, 512 MiB of input, which is
too much for a test that runs with every suite; it is left out.
"""

import functools

import numpy as np
import pytest

import cvt_reference as cr
import mx_reference as mx
from probe_gpu import _gpu
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)
from test_gpu_cvt_exact import SCALED, _assert_codes, _codes

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def _to(dev, x, rows, k):
    return torch.from_numpy(np.ascontiguousarray(x).reshape(rows, k).copy()).to(dev)


def _assert_quantize(what, dev, name, x, rows, k):
    """``mx_quantize`` of ``x`` as ``[rows, k]`` is the model's, scales and codes; and with those scales the
    bare instruction is the model's encoder, which differs from it exactly where the model saturated."""
    fmt = cr.NAMES[name]
    x = np.ascontiguousarray(x).reshape(rows, k)
    with np.errstate(invalid="ignore", over="ignore"):
        want_codes, want_scales = cr.quantize(fmt, x)
        want_raw = cr.encode(fmt, x, np.repeat(want_scales, 32, axis=1))
    tx = _to(dev, x, rows, k)
    codes, scales = _gpu().mx_quantize(name, tx)
    assert codes.dtype == scales.dtype == torch.uint8
    assert tuple(codes.shape) == want_codes.shape and tuple(scales.shape) == want_scales.shape
    got_scales = scales.cpu().numpy()
    if not np.array_equal(got_scales, want_scales):
        bad = np.flatnonzero(got_scales.reshape(-1) != want_scales.reshape(-1))
        first = [(int(b), int(got_scales.reshape(-1)[b]), int(want_scales.reshape(-1)[b])) for b in bad[:8]]
        pytest.fail(f"{what}: {len(bad)} of {want_scales.size} scales differ; (block, got, want) {first}")
    _assert_codes(f"{what} codes", _codes(name, codes), mx.unpack(fmt, want_codes).astype(np.int64), x)
    raw = _gpu().cvt_encode(name, tx, scales)
    _assert_codes(f"{what} raw", _codes(name, raw), want_raw, x)
    return want_codes, want_scales, want_raw


# ------------------------------------------------------------------ every binade of amax


FIELDS, KINDS = 255, 4  # exponent fields 0 … 254, four top mantissas each


@functools.lru_cache(maxsize=None)
def _binade_blocks():
    """One block per exponent field 0 … 254 and kind: ``[1020, 32]`` f32.  The block's top element has that
    exponent field and the kind's mantissa (field 0, the subnormals: 1, 1 << 7, 1 << 14, 0x7FFFFF; otherwise 0,
    0x7FFFFF, 0x400000, a seeded one), sits at (5 · field + kind) mod 32 and alternates in sign.  The other 31
    are seeded bit patterns up to 11 binades below it; one above the top becomes the top's bits >> 1."""
    rng = np.random.default_rng(2024)
    field, kind = np.divmod(np.arange(FIELDS * KINDS, dtype=np.uint32), KINDS)
    seeded = rng.integers(0, 1 << 23, FIELDS * KINDS, dtype=np.uint32)
    mant = np.where(field == 0, np.choose(kind, [1, 1 << 7, 1 << 14, 0x7FFFFF]),
                    np.choose(kind, [0, 0x7FFFFF, 0x400000, seeded])).astype(np.uint32)
    top = (field << 23) | mant
    down = rng.integers(0, 12, size=(len(top), 32), dtype=np.uint32)
    ef = np.where(down > field[:, None], 0, field[:, None] - down).astype(np.uint32)
    mag = (ef << 23) | rng.integers(0, 1 << 23, size=(len(top), 32), dtype=np.uint32)
    mag = np.where(mag > top[:, None], top[:, None] >> 1, mag)
    sign = rng.integers(0, 2, size=(len(top), 32), dtype=np.uint32)
    at = (5 * field + kind) % 32
    rows = np.arange(len(top))
    mag[rows, at] = top
    sign[rows, at] = (field + kind) & 1
    x = _f32((sign << 31) | mag)
    assert np.isfinite(x).all() and (np.abs(x).max(axis=1) == _f32(top)).all()
    return x


@pytest.mark.parametrize("name", SCALED)
def test_quantize_at_every_binade_of_amax(dev, name):
    fmt = cr.NAMES[name]
    x = _binade_blocks()
    cmax, sign = cr.CMAX[fmt], 1 << cr.sign_bit(fmt)
    for rows, k in ((1020, 32), (340, 96)):
        want_codes, want_scales, _ = _assert_quantize(f"{name} {rows}x{k}", dev, name, x, rows, k)
        # what the model alone must meet for the input to be the one intended
        assert want_scales.min() == 0 and want_scales.max() == 254 - cr.emax(fmt)
        assert {cr.FP8: 246, cr.BF8: 239, cr.FP4: 252, cr.FP6: 252, cr.BF6: 250}[fmt] == 254 - cr.emax(fmt)
        assert (want_scales == 0).sum() >= 12
        codes = mx.unpack(fmt, want_codes).astype(np.int64)
        assert ((codes & ~sign) <= cmax).all()  # no NaN and no infinity code
        assert (codes == cmax).any() and (codes == (cmax | sign)).any()
        assert np.array_equal(np.unique(want_scales), np.arange(0, 255 - cr.emax(fmt)))  # and every byte between


# ------------------------------------------------------------------ scale bytes 0 and 255 as operands


@pytest.mark.parametrize("name", SCALED)
def test_encode_of_every_high_half_at_scale_bytes_0_and_255(dev, name):
    """All 65536 f32 whose low 16 bits are zero at the two scale bytes ``test_gpu_cvt_exact`` leaves out: 0,
    whose operand is the f32 +0.0 and which means 2^-127, and 255, the E8M0 NaN, which makes every input a NaN
    input."""
    fmt = cr.NAMES[name]
    x = _f32(np.arange(65536, dtype=np.uint32) << 16)
    tx = _to(dev, x, 2048, 32)
    for byte in (0, 255):
        sc = torch.full((2048, 1), byte, dtype=torch.uint8, device=dev)
        with np.errstate(over="ignore", invalid="ignore"):
            want = cr.encode(fmt, x, byte)
        assert want.shape == (65536,)
        _assert_codes(f"{name} scale byte {byte}", _codes(name, _gpu().cvt_encode(name, tx, sc)).reshape(-1), want, x)
    signed = 0 if fmt in cr.NAN_CODE else np.signbit(x).astype(np.int64) << cr.sign_bit(fmt)
    assert (want == cr.SCALE_NAN_CODE[fmt] | signed).all()  # what a NaN input gives, whatever the input
    with np.errstate(over="ignore", invalid="ignore"):
        at0 = cr.encode(fmt, x, 0) & ~(1 << cr.sign_bit(fmt))
    sub = (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)
    assert at0[sub].any() and at0[sub].max() < cr.CMAX[fmt]  # f32 subnormals are values at byte 0, not all zeros


# ------------------------------------------------------------------ non-finite input to the quantiser


NONFINITE_BLOCKS = 1029  # nine workgroups of the 8-lane path, two of the 6-bit path, and a short last slab


@functools.lru_cache(maxsize=None)
def _nonfinite_blocks():
    """``[1029, 32]`` f32: the listed cases first, then seeded finite blocks with non-finite elements put in."""
    rng = np.random.default_rng(77)
    inf, flt_max = np.float32(np.inf), np.finfo(np.float32).max
    nans = _f32([0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000])  # payload in the low bits only, and quiet

    def finite(n):
        return (rng.standard_normal((n, 32)) * 2.0 ** rng.integers(-30, 30, size=(n, 1))).astype(np.float32)

    blocks = []
    b = np.zeros((1, 32), dtype=np.float32)
    b[0, 13] = inf
    blocks.append(b)  # +Inf alone in a block of zeros
    b = finite(4)
    b[0, 3], b[1, 30], b[2, 0], b[2, 31], b[3, 5], b[3, 6] = inf, -inf, inf, -inf, -inf, -inf
    blocks.append(b)  # ±Inf among finite values
    b = finite(8)
    for i in range(4):
        b[i, 7 * i + 2] = nans[i]  # one NaN of each sign and kind
        b[4 + i, [1, 18]] = nans[i], nans[3 - i]  # and two
    blocks.append(b)
    for nan in (nans[0], nans[3]):
        b = finite(32)
        b[np.arange(32), np.arange(32)] = nan  # a NaN at each of the 32 positions
        blocks.append(b)
    blocks.append(np.full((1, 32), nans[0]))  # all NaN
    blocks.append(np.full((1, 32), nans[3]))
    b = np.full((2, 32), nans[2])
    b[0, ::2], b[1, 5], b[1, 6::7] = inf, -inf, inf
    blocks.append(b)  # NaN and Inf only
    b = finite(4)
    b[0, 4], b[0, 20] = inf, flt_max
    b[1, 4], b[1, 20], b[1, 21] = -inf, -flt_max, flt_max
    b[2, 0], b[2, 9], b[2, 31] = nans[1], inf, flt_max
    b[3], b[3, 8] = flt_max, -inf
    blocks.append(b)  # Inf in blocks whose finite elements include FLT_MAX
    b = np.zeros((2, 32), dtype=np.float32)
    b[0, 9], b[1, 9], b[1, 10] = nans[0], nans[3], -0.0
    blocks.append(b)  # a NaN among zeros: nothing but zero counts
    listed = np.concatenate(blocks)
    rest = finite(NONFINITE_BLOCKS - len(listed))
    kind = np.arange(len(rest)) % 4  # 0: stays finite; 1: an Inf; 2: a NaN; 3: both
    has_inf, has_nan = np.flatnonzero(kind % 2 == 1), np.flatnonzero(kind >= 2)
    rest[has_inf, (has_inf * 5) % 32] = np.where(has_inf & 4, -inf, inf)
    rest[has_nan, (has_nan * 11 + 1) % 32] = nans[has_nan % 4]
    assert listed.shape[0] == 87
    x = np.concatenate([listed, rest])
    assert x.shape == (NONFINITE_BLOCKS, 32)
    return x


@pytest.mark.parametrize("name", SCALED)
def test_quantize_of_non_finite_blocks(dev, name):
    fmt = cr.NAMES[name]
    x = _nonfinite_blocks()
    cmax, sign = cr.CMAX[fmt], 1 << cr.sign_bit(fmt)
    want_codes, want_scales, want_raw = _assert_quantize(f"{name} non-finite", dev, name, x, NONFINITE_BLOCKS, 32)
    # the model does what the contract says of these blocks
    codes = mx.unpack(fmt, want_codes).astype(np.int64)
    isnan, isinf = np.isnan(x), np.isinf(x)
    assert isnan.any(axis=1).sum() > 400 and isinf.any(axis=1).sum() > 400 and (~np.isfinite(x)).all(axis=1).sum() == 4
    assert (want_scales != 255).all()
    assert (want_scales[isinf.any(axis=1), 0] == 254 - cr.emax(fmt)).all()
    assert (want_scales[isnan.all(axis=1), 0] == 127).all()
    assert (codes[isinf] == np.where(np.signbit(x[isinf]), cmax | sign, cmax)).all()
    if fmt in cr.NAN_CODE:
        assert (codes[isnan] == cr.NAN_CODE[fmt]).all() and ((codes[~isnan] & ~sign) <= cmax).all()
    else:
        assert (codes[isnan] == np.where(np.signbit(x[isnan]), cmax | sign, cmax)).all()
    assert (want_raw[isinf] & ~sign == cr.OVERFLOW[fmt][1]).all()  # the bare instruction does not saturate them
    # the same data three blocks to a row
    _assert_quantize(f"{name} non-finite 343x96", dev, name, x, NONFINITE_BLOCKS // 3, 96)


# ------------------------------------------------------------------ bf16


def test_bf16_of_every_high_half_with_six_low_halves(dev):
    """Subnormals, infinities, every NaN whose payload sits only in the low 16 bits (a truncating cast turns
    those into infinities), ties and their neighbours at every exponent: 393,216 values, NaN codes compared
    as bits."""
    low = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    x = _f32(((np.arange(65536, dtype=np.uint32) << 16)[:, None] | low[None, :]).reshape(-1))
    assert x.size == 393216 and np.isnan(x).sum() > 1500 and np.isinf(x).sum() == 2
    want = cr.encode(cr.BF16, x)
    only_low = np.isnan(x) & ((x.view(np.uint32) >> 16) & 0x7F == 0)
    assert only_low.sum() == 10 and (want[only_low] & 0x7FFF == 0x7FC0).all()
    tx = _to(dev, x, 384, 1024)
    enc = _gpu().cvt_encode("bf16", tx)
    q, scales = _gpu().mx_quantize("bf16", tx)
    assert scales is None and enc.dtype == q.dtype == torch.bfloat16 and tuple(q.shape) == (384, 1024)
    _assert_codes("bf16 cvt_encode", _codes("bf16", enc).reshape(-1), want, x)
    _assert_codes("bf16 mx_quantize", _codes("bf16", q).reshape(-1), want, x)


# ------------------------------------------------------------------ past the grid cap


CAP_ROWS, CAP_K = 524289, 32  # 4096 · 1024 + 8 pieces of 16 bytes: 64 MiB of input
PATTERN = 1 << 20


@functools.lru_cache(maxsize=None)
def _cap_pattern():
    """2^20 seeded f32 over 24 binades a block, both signs, every 16th block all zero."""
    rng = np.random.default_rng(4096)
    n = PATTERN // 32
    bits = (rng.integers(0, 2, (n, 32), dtype=np.uint32) << 31) | rng.integers(0, 1 << 23, (n, 32), dtype=np.uint32) \
        | ((rng.integers(90, 150, (n, 1), dtype=np.uint32) - rng.integers(0, 24, (n, 32), dtype=np.uint32)) << 23)
    bits[::16] = 0
    x = _f32(bits)
    assert np.isfinite(x).all()
    return x


def _tiled(t, rows):
    """The pattern's per-block result ``t`` ``[2^15, …]`` repeated to ``rows`` blocks."""
    return t.repeat(-(-rows // t.shape[0]), 1)[:rows].contiguous()


@pytest.mark.parametrize("name", ["fp8", "fp4", "bf16"])
def test_rows_kernel_beyond_the_grid_cap(dev, name):
    """With more than 4096 · 1024 pieces the grid stays at 4096 workgroups: slabs are 2048 pieces, the
    workgroups from 2049 on start beyond the end and the last busy one has 8 pieces.  The input is the pattern
    tiled, so the expected result is the model's result of the pattern tiled the same way."""
    fmt = cr.NAMES[name]
    assert CAP_ROWS * CAP_K // 4 == 4096 * 1024 + 8 and PATTERN // 32 * 16 + 1 == CAP_ROWS
    p = _cap_pattern()
    x = _tiled(torch.from_numpy(p).to(dev), CAP_ROWS)
    assert tuple(x.shape) == (CAP_ROWS, CAP_K)
    want_codes, want_scales = cr.quantize(fmt, p)

    def check(what, got, want):
        want = _tiled(torch.from_numpy(want).to(dev), CAP_ROWS)
        got = got.view(want.dtype)
        assert got.shape == want.shape, what
        if not torch.equal(got, want):
            bad = (got != want).any(dim=1).nonzero().reshape(-1)
            pytest.fail(f"{name} {what}: {len(bad)} of {CAP_ROWS} blocks differ, the first at {bad[:8].tolist()}, "
                        f"the last at {bad[-1].item()}")

    codes, scales = _gpu().mx_quantize(name, x)
    if name == "bf16":
        assert scales is None
        check("mx_quantize", codes, want_codes.view(np.int16))
        check("cvt_encode", _gpu().cvt_encode(name, x), want_codes.view(np.int16))
        return
    check("mx_quantize scales", scales, want_scales)
    check("mx_quantize codes", codes, want_codes)
    raw = mx.pack(fmt, cr.encode(fmt, p, np.repeat(want_scales, 32, axis=1)).astype(np.uint8))
    # some element of the pattern saturates, which the bare fp8 instruction does not do
    assert np.array_equal(raw, want_codes) == (cr.OVERFLOW[fmt][1] == cr.CMAX[fmt])
    check("cvt_encode codes", _gpu().cvt_encode(name, x, _tiled(torch.from_numpy(want_scales).to(dev), CAP_ROWS)), raw)
