"""Sweeps of the low-precision probe kernels on a real MI355X: ``mx_gemm256_kernel<FP8|FP4>``
(``gpu_probe_mx.h``) and ``dense_gemm256_kernel<F16|I8>`` (``gpu_probe_dense.h``), held to the
standard of the bf16 sweep of ``test_gpu_kernels_exact.py``.  The sweep and store checks are those
of ``probe_gpu.py``; ``test_gpu_mx_formats_exact.py`` runs them on BF8, FP6 and BF6.

* The fused check: one operand element per row and per column, and one scale byte per row and
  per column, is changed, launch by launch, at 2 × 2 tiles and several stages.  Every launch must
  count exactly the mismatches of the host model (the product of the corrupted operands against
  the table) and attribute them to the XCDs its own ``tile_xcd`` map names.
* NaN and inf operands are counted in every column of their row.
* The store kernels: every FP8 code against every FP8 code, every FP4 code against every FP4
  code, 256 half values against each other, and every E8M0 scale byte 1 .. 254, as one-hot
  products that are exact whatever the order of summation.

Everything is bit-exact.  The tests corrupt data only; every pointer handed to a kernel comes
from a torch allocation of exactly the size the shape implies (a launch's counter row and tile
map are rows of such an allocation).
"""

import numpy as np
import pytest

import probe_reference as ref
from probe_gpu import _assert_operands_are_the_models, _assert_store_exact, _gpu, _probe
from probe_gpu import store_applies_every_scale_byte, store_decodes_every_code, sweep_every_row_and_column
from probe_gpu import sweep_every_scale_byte
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MX_FORMATS = ["fp8", "fp4"]  # BF8, FP6 and BF6 run the same sweeps in test_gpu_mx_formats_exact.py
FORMATS = MX_FORMATS + ["f16", "i8"]


# ------------------------------------------------------------------ 1. every row and column


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_check_sees_every_row_and_column(dev, fmt, rows):
    sweep_every_row_and_column(fmt, rows)


# ------------------------------------------------------------------ 2. every scale byte position


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_fused_check_reads_every_scale_byte(dev, fmt, rows):
    sweep_every_scale_byte(fmt, rows)


# ------------------------------------------------------------------ 3. NaN and inf are counted

# row 173 = 128 (wave row 1) + 32 (fragment 1) + 8 (register group 1) + 4 (lane half 1) + 1:
# accumulator register 5 of the upper lane half
NAN_ROW = 173
NAN_CASES = [("fp8", 0x7F), ("f16", 0x7E00), ("f16", 0x7C00)]


@pytest.mark.parametrize("fmt,bits", NAN_CASES, ids=["fp8-nan", "f16-nan", "f16-inf"])
def test_fused_check_counts_nan_and_inf(dev, fmt, bits):
    """One element of A becomes NaN (or, f16, +inf): its row is wrong in all N columns — inf where
    ``Bt[j][k]`` is non-zero, NaN (inf · 0) where it is zero — and ``errors == N``."""
    gpu = _gpu()
    k = 2 * (64 if fmt == "fp8" else 32)
    p = _probe(fmt, 256, 256, k)
    i, kk = NAN_ROW, k - 3  # in the second stage
    row = i % 32  # row of the 32 × 32 fragment = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    assert (row & 3) + 4 * (row >> 3) == 5 and (row >> 2) & 1 == 1  # register 5, lane half 1
    host = p.host["a"].copy()
    if fmt == "fp8":
        host[i, kk] = bits
    else:
        host.view(np.uint16)[i, kk] = bits
    with np.errstate(invalid="ignore"):
        mismatch = p.product(dict(p.host, a=host)) != p.expect
    assert mismatch[i].all() and int(mismatch.sum()) == p.n
    if bits == 0x7C00:
        assert (p.values[1][:, kk] == 0).any() and (p.values[1][:, kk] != 0).any()  # both inf and NaN occur
    a = p.t["a"]
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    tile_xcd = torch.full((1,), -1, dtype=torch.int32, device=dev)
    clean = a[i, kk:kk + 1].clone()
    try:
        a[i, kk:kk + 1].copy_(torch.from_numpy(host[i, kk:kk + 1].copy()))
        p.launch(tile_xcd.data_ptr(), counters.data_ptr())
    finally:
        a[i, kk:kk + 1].copy_(clean)
    h = counters.cpu().tolist()
    xcd = int(tile_xcd.cpu()[0])
    _assert_operands_are_the_models(p)
    assert 0 <= xcd < gpu.N_XCD
    assert h[gpu.ODH_SLOT_GEMM_ERR] == p.n, h
    want_xcd = [p.n if x == xcd else 0 for x in range(gpu.N_XCD)]
    assert h[gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.N_XCD] == want_xcd, h
    assert h[gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + gpu.N_XCD] == [int(x == xcd) for x in range(gpu.N_XCD)]


# ------------------------------------------------------------------ 4. store kernels: code against code


@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_mx_store_decodes_every_code_against_every_code(dev, fmt):
    store_decodes_every_code(dev, fmt)


def test_mx_store_applies_every_scale_byte(dev):
    store_applies_every_scale_byte(dev, "fp8")


def test_f16_store_multiplies_every_value_by_every_value(dev):
    """256 halves — the integers, ±65504, the smallest normal, ±0, all-ones mantissas and random
    normals — against each other: each output one product, exact in fp32."""
    a, bt, want = ref.f16_onehot_case()
    c = torch.full(want.shape, 3e38, dtype=torch.float32, device=dev)
    _gpu().dense_gemm("f16", torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev), out=c)
    _assert_store_exact("f16 value i × value j", c.cpu().numpy(), want)
