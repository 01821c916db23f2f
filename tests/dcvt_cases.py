"""Cases and comparisons for the decoding converters (``test_dcvt_cases.py``, ``test_gpu_dcvt_edges.py``), next to
``mx_reference.py``: the reference of ``test_gpu_dcvt.py`` under its public name, the case that puts every code at
every scale byte into every position of a lane's load, the seeded pattern of the test beyond the grid cap, and the
comparisons, which say where a result differs.

The builders and the reference are numpy and torch on the host and make no GPU call.  The comparisons take what a
test read back; the one of whole blocks compares integer tensors on the device they are on.  Cases are built once
and shared: nobody writes to what these functions return.
"""

import functools

import numpy as np
import pytest
import torch

import mx_reference as ref
from test_gpu_dcvt import _bits as expected_bits

INF = {torch.float32: 0x7F800000, torch.float16: 0x7C00, torch.bfloat16: 0x7F80}
# places a code can take in what a lane of dcvt_rows_kernel loads: the byte's of the 8-byte load (its 4-byte load is
# either half), the nibble's of the 4-byte load (its 2-byte load likewise), the element's of a 6-bit block
POSITIONS = {"fp8": 8, "bf8": 8, "fp4": 8, "fp6": 32, "bf6": 32}


def scaled_values(fmt, codes, byte):
    """``value(code) · 2^(byte - 127)`` in float64, ``codes`` and ``byte`` broadcast; NaN where the byte is 255, the
    E8M0 NaN, zero and infinity codes included."""
    byte = np.asarray(byte, dtype=np.int64)
    v = ref.code_values(ref.NAMES[fmt])[np.asarray(codes, dtype=np.int64)] * 2.0 ** (byte - 127).astype(np.float64)
    return np.where(byte == 255, np.nan, v)


# ------------------------------------------------------------------ comparisons


def bits_of(t, dtype):
    """A tensor of ``dtype`` as the integers ``expected_bits`` gives."""
    return t.contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16).cpu().numpy().astype(np.int64)


def differing(got, values, dtype):
    """Flat indices at which the bits ``got`` are not the reference of ``values``: a NaN is compared by class,
    everything else bit for bit, ``-0`` and subnormals included.  Also ``got`` and the expected bits, in ``values``' shape."""
    want, nan = expected_bits(values, dtype)
    got = np.asarray(got, dtype=np.int64).reshape(want.shape)
    mag = 0x7FFFFFFF if dtype == torch.float32 else 0x7FFF
    return np.flatnonzero(np.where(nan, (got & mag) <= INF[dtype], got != want).ravel()), got, want


def assert_equals_reference(what, got, values, dtype, where=lambda i: f"element {i}"):
    """Fails with the number of differing elements and, for the first eight, ``where(flat index)``, got and want."""
    bad, got, want = differing(got, values, dtype)
    if bad.size == 0:
        return
    digits = 8 if dtype == torch.float32 else 4
    nan = np.isnan(np.asarray(values, dtype=np.float64)).ravel()
    first = [f"{where(int(i))} got 0x{int(got.ravel()[i]) & (1 << 4 * digits) - 1:0{digits}x} want "
             + ("a NaN" if nan[i] else f"0x{int(want.ravel()[i]) & (1 << 4 * digits) - 1:0{digits}x}") for i in bad[:8]]
    pytest.fail(f"{what}: {bad.size} of {want.size} elements differ: " + "; ".join(first))


def triple_of(fmt, codes, scales):
    """For operands in the public layout, a function of an element's flat index that names its (code, scale byte,
    position)."""
    c = ref.unpack(ref.NAMES[fmt], codes)
    k = c.shape[1]

    def where(i):
        row, j = divmod(i, k)
        return f"(code 0x{int(c[row, j]):02x}, scale byte {int(scales[row, j // 32])}, position {j % POSITIONS[fmt]})"

    return where


def tiled(t, rows):
    """The per-block tensor ``t`` ``[blocks, …]`` repeated to ``rows`` blocks."""
    return t.repeat(-(-rows // t.shape[0]), 1)[:rows].contiguous()


def assert_blocks_equal(what, got, want):
    """Integer tensors ``[blocks, …]`` on one device: how many blocks differ, the first and the last."""
    assert got.shape == want.shape and got.dtype == want.dtype and not got.dtype.is_floating_point, what
    if not torch.equal(got, want):
        bad = (got != want).any(dim=1).nonzero().reshape(-1)
        pytest.fail(f"{what}: {len(bad)} of {got.shape[0]} blocks differ, the first at {bad[:8].tolist()}, "
                    f"the last at {bad[-1].item()}")


GUARD, GUARD_FILL = 64 << 10, 0xA5


def assert_guards_untouched(what, buf, nbytes):
    """``buf``: uint8, filled with ``GUARD_FILL`` before a kernel wrote ``nbytes`` from byte ``GUARD`` on.  Every
    byte before and after those is still the fill."""
    hit = np.flatnonzero(buf.cpu().numpy() != GUARD_FILL)
    hit = hit[(hit < GUARD) | (hit >= GUARD + nbytes)] - GUARD
    if hit.size:
        pytest.fail(f"{what}: {hit.size} bytes written outside out[0:{nbytes}], at offsets {hit[:8].tolist()} "
                    f"… {int(hit[-1])}")


# ------------------------------------------------------------------ every code, every scale byte, every position

EVERY_PAIR = {"fp8": (256, 8), "bf8": (256, 8), "fp4": (64, 8), "fp6": (64, 32), "bf6": (64, 32)}  # K, rotations


@functools.lru_cache(maxsize=None)
def every_pair_case(fmt):
    """Codes ``[rows, mx_row_bytes]``, scales ``[rows, K/32]`` and the float64 values ``[rows, K]``.  Row
    ``b · rotations + rot`` (``b`` 0 … 255) holds code ``(j + rot) mod ncodes`` in element ``j`` and scale byte
    ``(b + 37 t) & 255`` on block ``t``: a code meets every position through ``rot`` and every scale byte through
    ``b``, and 37 being odd no two neighbouring blocks share a byte."""
    k, nrot = EVERY_PAIR[fmt]
    name = ref.NAMES[fmt]
    ncodes, npos = 1 << ref.code_bits(name), POSITIONS[fmt]
    b, rot = np.divmod(np.arange(256 * nrot), nrot)
    codes = (np.arange(k)[None, :] + rot[:, None]) % ncodes
    scales = ((b[:, None] + 37 * np.arange(k // 32)[None, :]) & 255).astype(np.uint8)
    byte = np.repeat(scales.astype(np.int64), 32, axis=1)
    values = scaled_values(fmt, codes, byte)
    triples = (codes * 256 + byte) * npos + np.arange(k)[None, :] % npos
    assert np.unique(triples).size == ncodes * 256 * npos, "every (code, scale byte, position)"
    flat = scales.reshape(-1)
    assert (flat[1:] != flat[:-1]).all(), "neighbouring blocks, across rows too, differ in their scale byte"
    # a block in 256 has byte 255; of the others, the format's NaN codes: each (rot, j) meets every b once
    nan_codes = int(np.isnan(ref.code_values(name)).sum())
    assert nan_codes == {"fp8": 2, "bf8": 6}.get(fmt, 0)
    assert int(np.isnan(values).sum()) * 256 * ncodes == values.size * (ncodes + 255 * nan_codes)
    return ref.pack(name, codes), scales, values


# ------------------------------------------------------------------ seeded blocks whose result bits are determined


def determined_case(fmt, rows, k, seed):
    """Seeded codes ``[rows, mx_row_bytes]``, scales ``[rows, K/32]`` and values ``[rows, K]`` with no NaN result: no
    fp8 or bf8 NaN code (bf8's infinities stay in), scale bytes 0 … 254, and every 16th block all zero codes."""
    name = ref.NAMES[fmt]
    rng = np.random.default_rng(seed)
    allowed = np.flatnonzero(~np.isnan(ref.code_values(name)))
    codes = rng.choice(allowed, (rows * k // 32, 32))
    codes[::16] = 0
    scales = rng.integers(0, 255, (rows, k // 32), dtype=np.uint8)
    codes = codes.reshape(rows, k)
    values = scaled_values(fmt, codes, np.repeat(scales.astype(np.int64), 32, axis=1))
    assert not np.isnan(values).any()
    return ref.pack(name, codes), scales, values


CAP_PATTERN = 1 << 15  # blocks


@functools.lru_cache(maxsize=None)
def cap_pattern(fmt):
    """``determined_case`` of 2^15 blocks (K = 32), for the test beyond the grid cap: its expected bits, tiled, are
    compared as integers."""
    codes, scales, values = determined_case(fmt, CAP_PATTERN, 32, seed=4096)
    assert np.array_equal(np.unique(scales), np.arange(255))
    assert not values[::16].any() and (np.isinf(values).any() == (fmt == "bf8"))
    return codes, scales, values


# ------------------------------------------------------------------ one instruction


def one_instruction_cases(fmt, form):
    """The launches of ``test_one_instruction_equals_the_table``: ``(src, sel, codes)`` with ``src`` the int32 source
    registers of the 64 lanes and ``codes[l]`` the codes whose values lane ``l`` returns.  6-bit: code ``(l + k) & 63``
    at position ``k``, every code in every position.  Otherwise byte value ``64 t + l`` in byte 0 of lane ``l`` and other
    values in the other bytes, for ``t`` 0 … 3, through every select."""
    lanes = np.arange(64)
    if fmt in ("fp6", "bf6"):
        codes = (lanes[:, None] + np.arange(32)) & 63
        yield np.ascontiguousarray(ref.pack6(codes)).view(np.int32), 0, codes
        return
    for t in range(4):
        by = (64 * t + lanes[:, None] + 85 * np.arange(4)) & 255
        src = (by << (8 * np.arange(4))).sum(axis=1).astype(np.uint32).view(np.int32)
        for sel in range(4 if fmt == "fp4" or form == 1 else 2):
            if fmt == "fp4":
                codes = np.stack([by[:, sel] & 15, by[:, sel] >> 4], axis=1)
            else:
                codes = by[:, sel:sel + 1] if form == 1 else by[:, 2 * sel:2 * sel + 2]
            yield src, sel, codes
