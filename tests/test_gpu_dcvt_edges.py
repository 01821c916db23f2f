"""``mx_dequantize`` and the decoding converters on a real MI355X against the reference (``dcvt_cases.py``) where
``test_gpu_dcvt.py`` does not go: every code at every scale byte in every position of a lane's load; one instruction
at a time at the scale bytes outside the exact window (subnormal results, rounding into float16, overflow, bytes 0
and 255), the one-value form and fp4's byte selects 2 and 3 included; a scale operand with mantissa and sign bits;
piece counts at every edge of the row kernel's 4-deep unroll, into an output with guards on both sides; codes at
8 mod 16 bytes and scales at an odd address; and shapes beyond the grid cap of 4096 workgroups, where slabs grow past
1024 pieces, the loop runs twice and the trailing workgroups have nothing to do.

Everything is bit-exact, a NaN compared by class.  Nothing is filtered afterwards.  The tests feed data only: every
pointer handed to a kernel lies inside a torch allocation that holds everything the shape implies.

Beyond the cap only the 8-lane path is run, once per width of its loads (fp8 and fp4, to float32 and to 16 bits).
The 6-bit path counts blocks, not pieces: its cap lies at 4096 · 1024 blocks, at least 256 MiB of output, which is too
much for a test that runs with every suite; it is left out.  Its loop and slabs are the same template on the same
``slab_of``.
"""

import numpy as np
import pytest
import torch

import dcvt_cases as dc
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)
from test_gpu_dcvt import DTYPES, FORMATS, ONE, WINDOW
from odh_kubeflow_amd.ops import gpu

pytestmark = pytest.mark.gpu

IDS = ["f32", "f16", "bf16"]
DST = {torch.float32: gpu.ODH_DCVT_F32, torch.float16: gpu.ODH_DCVT_F16, torch.bfloat16: gpu.ODH_DCVT_BF16}


def _name(v):
    return str(v).replace("torch.", "")


def _window(fmt, dtype):
    return WINDOW[fmt, 16 if dtype == torch.float16 else 32]


# ------------------------------------------------------------------ every code, scale byte and position


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_dequantize_of_every_code_at_every_scale_byte(dev, fmt, dtype):
    codes, scales, values = dc.every_pair_case(fmt)
    out = gpu.mx_dequantize(fmt, torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev), dtype)
    assert out.dtype == dtype and tuple(out.shape) == values.shape
    dc.assert_equals_reference(f"{fmt} to {_name(dtype)}", dc.bits_of(out, dtype), values, dtype,
                               dc.triple_of(fmt, codes, scales))


# ------------------------------------------------------------------ one instruction outside the window


def _one(dev, fmt, dtype, form, operand, byte):
    """Every launch of ``one_instruction_cases`` with the scale operand ``operand`` in all lanes, against the reference
    of scale byte ``byte``."""
    scale = torch.from_numpy(np.full(64, operand, dtype=np.uint32).view(np.int32)).to(dev)
    for src, sel, codes in dc.one_instruction_cases(fmt, form):
        got = gpu.dcvt_one(fmt, dtype, torch.from_numpy(src).to(dev), scale, sel=sel, form=form)
        dc.assert_equals_reference(
            f"{fmt} to {_name(dtype)} form {form} select {sel} operand 0x{operand:08x}", dc.bits_of(got, dtype),
            dc.scaled_values(fmt, codes, byte), dtype,
            lambda i: f"(lane {i // codes.shape[1]}, code 0x{int(codes.ravel()[i]):02x}, scale byte {byte})")


@pytest.mark.parametrize("fmt, dtype, form", ONE, ids=_name)
def test_one_instruction_at_the_scale_bytes_outside_the_window(dev, fmt, dtype, form):
    """The window's last bytes and the first ones outside it, the ends of the finite range and the E8M0 NaN; for bf8 to
    float16, which has no window, the bytes where e5m2's smallest and largest codes leave float16 (112, 142)."""
    window = _window(fmt, dtype)
    if window is None:
        assert (fmt, dtype) == ("bf8", torch.float16)
        bytes_ = {0, 1, 112, 127, 142, 254, 255}
    else:
        lo, hi = window
        bytes_ = {0, 1, lo - 1, lo, hi, hi + 1, 254, 255}
    for byte in sorted(bytes_):
        _one(dev, fmt, dtype, form, byte << 23, byte)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_scale_operand_mantissa_and_sign_are_ignored(dev, fmt, dtype):
    """Only the exponent field of the float32 scale operand counts: with mantissa bits (the lowest, the highest, all)
    and with the sign bit the result is the reference of the byte, at the window's two ends too."""
    window = _window(fmt, dtype)
    for byte in sorted({127} | set(window or ())):
        for mant in (1, 0x400000, 0x7FFFFF):
            for sign in (0, 1 << 31):
                _one(dev, fmt, dtype, 0, sign | byte << 23 | mant, byte)


# ------------------------------------------------------------------ the row kernel's unroll, stores and loads


def _pieces_per_block(fmt, dtype):
    """Pieces of the row kernel in a block of 32: 16 bytes of the output, or the block itself (6-bit formats)."""
    return 1 if fmt in ("fp6", "bf6") else 8 if dtype == torch.float32 else 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_kernel_at_the_edges_of_the_unroll(dev, fmt, dtype):
    """A lane's four pieces lie 256 apart and a slab is 1024 pieces: one block, and one block less than, exactly and
    one block more than 256, 512, 768, 1024 and 1280 pieces.  The output lies between two guards inside one
    allocation, so a piece stored too far, or too early, is counted instead of lost."""
    per = _pieces_per_block(fmt, dtype)
    edges = [1] + [m // per + d for m in (256, 512, 768, 1024, 1280) for d in (-1, 0, 1)]
    assert all(e >= 1 for e in edges) and len(set(edges)) == 16
    top = max(edges)
    codes, scales, values = dc.determined_case(fmt, top, 32, seed=top)
    tc, ts = torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev)
    size = 4 if dtype == torch.float32 else 2
    buf = torch.empty((dc.GUARD + top * 32 * size + dc.GUARD,), dtype=torch.uint8, device=dev)
    assert (buf.data_ptr() + dc.GUARD) % 16 == 0 and tc.data_ptr() % 8 == 0
    lib, stream = gpu.load_library(), torch.cuda.current_stream(dev).cuda_stream
    for rows in edges:
        nbytes = rows * 32 * size
        buf.fill_(dc.GUARD_FILL)
        gpu._check(lib.odh_mx_dequantize(gpu.DCVT_FORMATS[fmt], DST[dtype], tc.data_ptr(), ts.data_ptr(),
                                         buf.data_ptr() + dc.GUARD, rows, 32, stream))
        what = f"{fmt} to {_name(dtype)}, {rows} blocks ({rows * per} pieces)"
        out = buf[dc.GUARD:dc.GUARD + nbytes].view(dtype).reshape(rows, 32)
        dc.assert_equals_reference(what, dc.bits_of(out, dtype), values[:rows], dtype, dc.triple_of(fmt, codes, scales))
        dc.assert_guards_untouched(what, buf, nbytes)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_codes_and_scales_at_an_offset(dev, fmt, dtype):
    """Codes that start 8 bytes past a multiple of 16, the least the 8-byte loads are promised, and scales at an odd
    address: both are the tail of a larger tensor, so every read stays inside an allocation of the test's."""
    if fmt in ("fp6", "bf6"):  # 24-byte rows: the second row starts at 8 mod 16
        rows, k = 1031, 32
        codes, scales, values = dc.determined_case(fmt, rows, k, seed=8)
        tc = torch.from_numpy(np.concatenate([codes[:1], codes])).to(dev)[1:]
    else:
        rows, k = 131, 96
        codes, scales, values = dc.determined_case(fmt, rows, k, seed=8)
        flat = torch.from_numpy(np.concatenate([np.zeros(8, dtype=np.uint8), codes.reshape(-1)])).to(dev)
        tc = flat[8:].view(rows, codes.shape[1])
    ts = torch.from_numpy(np.concatenate([scales[:1], scales])).to(dev)[1:]
    assert k // 32 % 2 == 1 and tc.data_ptr() % 16 == 8 and ts.data_ptr() % 2 == 1
    assert rows * k // 32 * _pieces_per_block(fmt, dtype) > 1024  # more than one workgroup
    out = gpu.mx_dequantize(fmt, tc, ts, dtype)
    dc.assert_equals_reference(f"{fmt} to {_name(dtype)}", dc.bits_of(out, dtype), values, dtype,
                               dc.triple_of(fmt, codes, scales))


# ------------------------------------------------------------------ past the grid cap

# the four widths of the 8-lane path's loads: 4 bytes, 2, 8 and 4
BEYOND = [("fp8", torch.float32, 524289), ("fp4", torch.float32, 524289), ("fp8", torch.bfloat16, 1048578),
          ("fp4", torch.float16, 1048578)]


@pytest.mark.parametrize("fmt, dtype, rows", BEYOND, ids=["fp8-f32", "fp4-f32", "fp8-bf16", "fp4-f16"])
def test_rows_kernel_beyond_the_grid_cap(dev, fmt, dtype, rows):
    """With 4096 · 1024 + 8 pieces the grid stays at 4096 workgroups: slabs are 2048 pieces and take two passes of the
    loop, the workgroups from 2049 on start beyond the end and the last busy one has 8 pieces.  The input is the
    pattern tiled, so the expected result is the reference of the pattern tiled the same way; 2^15 does not divide
    the rows, so the edges of the tiles are not those of the slabs."""
    assert rows * 32 // (4 if dtype == torch.float32 else 8) == 4096 * 1024 + 8 and rows % dc.CAP_PATTERN in (1, 2)
    codes, scales, values = dc.cap_pattern(fmt)
    bits, nan = dc.expected_bits(values, dtype)
    assert not nan.any()
    want = torch.from_numpy(bits.astype(np.int32 if dtype == torch.float32 else np.int16)).to(dev)
    out = gpu.mx_dequantize(fmt, dc.tiled(torch.from_numpy(codes).to(dev), rows),
                            dc.tiled(torch.from_numpy(scales).to(dev), rows), dtype)
    assert out.dtype == dtype and tuple(out.shape) == (rows, 32) and out.numel() * out.element_size() == (64 << 20) + 128
    dc.assert_blocks_equal(f"{fmt} to {_name(dtype)}", out.view(want.dtype), dc.tiled(want, rows))
