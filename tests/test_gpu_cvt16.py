"""``mx_quantize`` and ``cvt_encode`` of bfloat16 and float16 rows on a real MI355X (``ops/csrc/gpu_probe_cvt16.h``).

One sentence is the contract: for every 16-bit ``x``, ``mx_quantize(fmt, x)`` is ``mx_quantize(fmt, x.float())`` byte
for byte, so the reference is ``cvt_reference.quantize`` / ``.encode`` of the exactly widened values.  Inputs are built
as bit patterns and nothing is filtered afterwards.  Every pointer handed to a kernel comes from a torch allocation
that holds what the shape implies; the guard test hands in a larger one and looks behind the result.
"""

import numpy as np
import pytest
import torch

import cvt_reference as cr
import mx_reference as mx
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)
from odh_kubeflow_amd.ops import gpu

pytestmark = pytest.mark.gpu

FORMATS = ["fp8", "bf8", "fp4", "fp6", "bf6"]
SOURCES = {"bf16": (torch.bfloat16, 7, 254), "f16": (torch.float16, 10, 30)}  # dtype, mantissa bits, top finite field
both = pytest.mark.parametrize("fmt, src", [(f, s) for f in FORMATS for s in SOURCES])


def _rows(bits, src, shape, dev):
    """16-bit patterns as a tensor of the source type."""
    return torch.from_numpy(np.asarray(bits).astype(np.uint16).view(np.int16)).view(SOURCES[src][0]).reshape(shape).to(dev)


def _seeded(src, shape, dev, seed=16):
    """Finite values over sixteen binades a row of blocks, four within a block."""
    rng = np.random.default_rng(seed)
    nb = shape[0] * shape[1] // 32
    x = rng.standard_normal((nb, 32)) * 2.0 ** (rng.integers(-8, 8, (nb, 1)) - rng.integers(0, 4, (nb, 32)))
    return torch.from_numpy(x.reshape(shape)).to(SOURCES[src][0]).to(dev)


def _assert_quantize(fmt, x, got=None):
    with np.errstate(all="ignore"):
        want_codes, want_scales = cr.quantize(cr.NAMES[fmt], x.float().cpu().numpy())
    codes, scales = got if got is not None else gpu.mx_quantize(fmt, x)
    codes, scales = codes.cpu().numpy().reshape(want_codes.shape), scales.cpu().numpy().reshape(want_scales.shape)
    bad = np.argwhere(scales != want_scales)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), scales[scales != want_scales][:4], want_scales[scales != want_scales][:4])
    bad = np.argwhere(codes != want_codes)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), codes[codes != want_codes][:4], want_codes[codes != want_codes][:4])
    return want_codes, want_scales


@both
def test_every_source_value(dev, fmt, src):
    """All 65536 patterns, 31 consecutive ones to a block behind an anchor whose exponent field is theirs plus d:
    d = 0 lets the clamp act, the larger d push the patterns down through the destination's subnormals to zero."""
    _, mbits, top = SOURCES[src]
    p = (np.arange(2115 * 31) % 65536).reshape(-1, 31)
    field = (p[:, 0] & 0x7FFF) >> mbits
    x = np.concatenate([np.concatenate([(np.minimum(field + d, top) << mbits)[:, None], p], axis=1) for d in (0, 1, 3, 6, 12, 20)])
    _, scales = _assert_quantize(fmt, _rows(x, src, (-1, 32), dev))
    assert scales.max() == 254 - cr.emax(cr.NAMES[fmt])  # the blocks with an infinity


@both
def test_shapes_and_what_lies_behind_the_result(dev, fmt, src):
    """One block (a tail workgroup of the LDS kernel), odd block counts over a wave's edge, several slabs with a
    short last one, one block past a tile of 256; the bytes behind codes and scales keep their fill."""
    lib, code = gpu.load_library(), gpu.CVT_FORMATS[fmt]
    for rows, k in ((1, 32), (5, 160), (1031, 64), (257, 32)):
        x = _seeded(src, (rows, k), dev, seed=rows)
        nc, ns = rows * gpu.mx_row_bytes(fmt, k), rows * k // 32
        codes = torch.full((nc + 64,), 0xA5, dtype=torch.uint8, device=dev)
        scales = torch.full((ns + 64,), 0xA5, dtype=torch.uint8, device=dev)
        ctype = gpu.ODH_DCVT_BF16 if src == "bf16" else gpu.ODH_DCVT_F16
        assert lib.odh_cvt_quantize16(code, ctype, x.data_ptr(), codes.data_ptr(), scales.data_ptr(), rows, k,
                                      torch.cuda.current_stream(dev).cuda_stream) == 0
        _assert_quantize(fmt, x, (codes[:nc], scales[:ns]))
        assert (codes[nc:] == 0xA5).all() and (scales[ns:] == 0xA5).all(), (rows, k)
        _assert_quantize(fmt, x)


@both
def test_special_blocks(dev, fmt, src):
    _, mbits, top = SOURCES[src]
    inf, one = (top + 1) << mbits, (top // 2) << mbits
    x = np.full((6, 32), one, dtype=np.int64)
    x[0], x[1], x[4], x[5] = 0, inf | 1, 0x8000, 0  # all zero; all NaN; -0 only; below: amax a subnormal
    x[2, 9], x[3, 30], x[3, 2] = inf, 0x8000 | inf, top << mbits  # one +Inf, one -Inf, among finite values
    x[5, 3], x[5, 17] = 0x8003, 0x0002  # three quanta of 2^-24 (float16) or 2^-133: floor(log2) is one more
    _, scales = _assert_quantize(fmt, _rows(x, src, (6, 32), dev))
    emax = cr.emax(cr.NAMES[fmt])
    sub = max(0, 1 + (-24 if src == "f16" else -133) - emax + 127)
    assert scales.reshape(-1).tolist() == [127, 127, 254 - emax, 254 - emax, 127, sub] and (scales != 255).all()


@both
def test_encode_is_the_bare_instruction(dev, fmt, src):
    x = _seeded(src, (5, 160), dev)
    xf = x.float().cpu().numpy()
    sc = cr.mx_scales(cr.NAMES[fmt], xf).astype(np.int64) + 1  # so that no quotient exceeds the largest value
    assert sc.max() <= 254 and np.isfinite(xf).all()
    got = gpu.cvt_encode(fmt, x, torch.from_numpy(sc.astype(np.uint8)).to(dev))
    want = mx.pack(cr.NAMES[fmt], cr.encode(cr.NAMES[fmt], xf, np.repeat(sc, 32, axis=1)).astype(np.uint8))
    assert np.array_equal(got.cpu().numpy(), want)


@both
def test_dequantize_inverts_quantize(dev, fmt, src):
    """Values of the destination times a power of two that the source type holds exactly."""
    rng = np.random.default_rng(7)
    finite = mx.code_values(mx.NAMES[fmt])
    finite = finite[np.isfinite(finite) & (finite != 0)]
    x = rng.choice(finite, (9, 32))
    x[:, 0] = finite.max()  # the block's amax, so its scale is the power of two below
    x = (x * 2.0 ** rng.integers(*((-20, 21) if src == "bf16" else (-6, 1)), (9, 1))).reshape(3, 96)
    xt = torch.from_numpy(x).to(SOURCES[src][0]).to(dev)
    assert (xt.double().cpu().numpy() == x).all()
    assert torch.equal(gpu.mx_dequantize(fmt, *gpu.mx_quantize(fmt, xt), xt.dtype), xt)


def test_entry_points_check_before_launch(dev):
    x = torch.zeros((4, 64), dtype=torch.bfloat16, device=dev)
    s = torch.full((4, 2), 127, dtype=torch.uint8, device=dev)
    flat = torch.zeros(4 * 64 + 8, dtype=torch.float16, device=dev)
    for bad in (x.double(), x.to(torch.int16), flat[1:257].reshape(4, 64), x[:, :48].contiguous()):
        with pytest.raises(ValueError):
            gpu.mx_quantize("fp8", bad)
        with pytest.raises(ValueError):
            gpu.cvt_encode("fp6", bad, s)
    with pytest.raises(ValueError):
        gpu.mx_quantize("bf16", x)
    lib, st = gpu.load_library(), torch.cuda.current_stream(dev).cuda_stream
    out = torch.zeros((4, 64), dtype=torch.uint8, device=dev)
    px, ps, po = x.data_ptr(), s.data_ptr(), out.data_ptr()
    bf16, f32 = gpu.ODH_DCVT_BF16, gpu.ODH_DCVT_F32
    for args in ((5, bf16, px, ps, po, 4, 64), (9, bf16, px, ps, po, 4, 64), (0, f32, px, ps, po, 4, 64), (0, 3, px, ps, po, 4, 64),
                 (0, bf16, None, ps, po, 4, 64), (0, bf16, px, None, po, 4, 64), (0, bf16, px, ps, None, 4, 64),
                 (0, bf16, px + 8, ps, po, 2, 64), (0, bf16, px, ps, po + 4, 4, 64), (2, bf16, px, ps, po + 8, 4, 64),
                 (0, bf16, px, ps, po, 4, 48), (0, bf16, px, ps, po, 1 << 34, 64)):
        assert lib.odh_cvt_encode16(*args, st) != 0, args
        fmt, src, ax, asc, ao, r, kk = args
        assert lib.odh_cvt_quantize16(fmt, src, ax, ao, asc, r, kk, st) != 0, args
    torch.cuda.synchronize(dev)
    assert not out.any() and (s == 127).all()
