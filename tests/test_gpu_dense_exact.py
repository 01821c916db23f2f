"""The FP16 / INT8 probe kernels on a real MI355X against a host product:
``v_mfma_f32_32x32x16_f16`` and ``v_mfma_i32_32x32x32_i8`` through ``odh_dense_gemm``,
``odh_dense_fill``, ``odh_dense_probe_gemm_verify`` and ``odh-gpu-probe --dtypes``.

Everything is bit-exact.  Operands are integers; each case checks on the CPU that
``sum_k |a| |b|`` stays below ``2^24`` (f16: every partial sum is an integer fp32 holds) or
``2^31`` (i8: no int32 overflow), so the result is exact in any summation order.  The tests corrupt
data only; every pointer handed to a kernel comes from a torch allocation of exactly the size
the shape implies.
"""

import functools
import json

import numpy as np
import pytest

import probe_reference as ref
from probe_gpu import NP_DTYPE, _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = ["f16", "i8"]
EXACT_BELOW = {"f16": 2 ** 24, "i8": 2 ** 31}
I8_MUL_A, I8_MUL_B = 25, 41


def _stage(fmt):
    return 64 if fmt == "i8" else 32  # elements per 64-byte stage of a row


# ------------------------------------------------------------------ store kernel


@functools.lru_cache(maxsize=None)
def _random_case(fmt, m, n, k):
    """Seeded random operands (f16: the integers -8 .. 8; i8: the full range, -128 included) and
    their exact int64 product."""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + len(fmt))
    lo, hi = (-128, 128) if fmt == "i8" else (-8, 9)
    a = rng.integers(lo, hi, size=(m, k), dtype=np.int64)
    bt = rng.integers(lo, hi, size=(n, k), dtype=np.int64)
    if fmt == "i8":
        a[0, 0], bt[0, 0] = -128, -128  # the one product that overflows int16: +16384
    want = a @ bt.T
    # exact in any summation order: every partial sum stays below the accumulator's exact range
    assert (np.abs(a) @ np.abs(bt).T).max() < EXACT_BELOW[fmt]
    return a.astype(NP_DTYPE[fmt]), bt.astype(NP_DTYPE[fmt]), want


def _exact_store(dev, fmt, m, n, k):
    gpu = _gpu()
    a, bt, want = _random_case(fmt, m, n, k)
    if fmt == "i8":
        c = torch.full((m, n), -(2 ** 31), dtype=torch.int32, device=dev)
    else:
        c = torch.full((m, n), float("nan"), dtype=torch.float32, device=dev)
    gpu.dense_gemm(fmt, torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev), out=c)
    got = c.cpu().numpy().astype(np.float64)
    if not np.array_equal(got, want.astype(np.float64)):
        bad = np.argwhere(got != want)
        pytest.fail(f"{fmt} {m}x{n}x{k}: {len(bad)} wrong elements, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


# fewer than, equal to and more than the three stages in flight and the four ring slots, and a
# long K of 64 stages
K_STAGES = [1, 2, 3, 4, 5, 7, 64]
# one stage; workgroup counts = 0, 1 and 7 mod 8 (the XCD remap's three cases), then a single
# tile row of 11
GRIDS = [(512, 1024), (768, 768), (1280, 768), (256, 2816)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stages", K_STAGES)
def test_dense_gemm_exact_over_k(dev, fmt, stages):
    _exact_store(dev, fmt, 256, 256, stages * _stage(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", GRIDS)
def test_dense_gemm_exact_over_grids(dev, fmt, m, n):
    _exact_store(dev, fmt, m, n, _stage(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_gemm_exact_over_tiles_and_stages(dev, fmt):
    """2 × 3 tiles at 3 stages: operand addresses with a tile offset and ``kt > 0``."""
    _exact_store(dev, fmt, 512, 768, 3 * _stage(fmt))


# ------------------------------------------------------------------ entry points refuse


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_entry_points_check_before_launch(dev, fmt):
    gpu = _gpu()
    k = 2 * _stage(fmt)
    a, bt, _ = _random_case(fmt, 256, 256, k)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev)
    other = torch.float16 if fmt == "i8" else torch.int8
    for fn in (gpu.dense_gemm, gpu.dense_verify, gpu.dense_fill):
        with pytest.raises(ValueError):
            fn("bf16", ta, tb)
        with pytest.raises(TypeError):
            fn(fmt, ta.to(other), tb)
        with pytest.raises(TypeError):
            fn(fmt, ta, tb.to(torch.float32))
        with pytest.raises(ValueError):
            fn(fmt, ta.t(), tb)  # not contiguous
        with pytest.raises(ValueError):
            fn(fmt, ta[:, ::2], tb[:, ::2])  # not contiguous
        with pytest.raises(ValueError):
            fn(fmt, ta[:, :k // 4].contiguous(), tb[:, :k // 4].contiguous())  # K is half a stage
        with pytest.raises(ValueError):
            fn(fmt, ta[:128].contiguous(), tb)  # M = 128
        with pytest.raises(ValueError):
            fn(fmt, ta, tb[:, :k // 2].contiguous())  # K of A and of Bt differ
        with pytest.raises(ValueError):
            fn(fmt, ta.cpu(), tb)  # not on the same device
    good = torch.int32 if fmt == "i8" else torch.float32
    for out in (torch.empty((256, 256), dtype=torch.int32 if good == torch.float32 else torch.float32, device=dev),
                torch.empty((256, 128), dtype=good, device=dev), torch.empty((256, 256), dtype=good)):
        with pytest.raises(ValueError):
            gpu.dense_gemm(fmt, ta, tb, out=out)


def test_dense_c_abi_refuses_before_launch(dev):
    """The library's own checks, below the Python ones: ``hipErrorInvalidValue`` and no launch."""
    gpu = _gpu()
    lib = gpu.load_library()
    invalid = 1  # hipErrorInvalidValue
    a = torch.zeros((256, 128), dtype=torch.int8, device=dev)
    bt = torch.zeros((256, 128), dtype=torch.int8, device=dev)
    c = torch.zeros((256, 256), dtype=torch.int32, device=dev)
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pa, pb, pc, pk = a.data_ptr(), bt.data_ptr(), c.data_ptr(), counters.data_ptr()
    f16, i8 = gpu.ODH_DT_F16, gpu.ODH_DT_I8
    for args in ((0, pa, pb, pc, 256, 256, 128), (3, pa, pb, pc, 256, 256, 128),  # unknown formats
                 (i8, pa, pb, pc, 128, 256, 128), (i8, pa, pb, pc, 256, 384, 128), (i8, pa, pb, pc, 256, 256, 32),
                 (f16, pa, pb, pc, 256, 256, 16), (i8, pa, pb, pc, 256, 256, 0),
                 (i8, None, pb, pc, 256, 256, 128), (i8, pa, None, pc, 256, 256, 128),
                 (i8, pa + 8, pb, pc, 256, 256, 64), (i8, pa, pb + 4, pc, 256, 256, 64)):  # not 16-byte aligned
        fmt, xa, xb, xc, m, n, k = args
        assert lib.odh_dense_gemm(fmt, xa, xb, xc, m, n, k, s) == invalid, args
        assert lib.odh_dense_fill(fmt, xa, xb, m, n, k, s) == invalid, args
        assert lib.odh_dense_probe_gemm_verify(fmt, xa, xb, m, n, k, None, pk, s) == invalid, args
    assert lib.odh_dense_gemm(i8, pa, pb, None, 256, 256, 128, s) == invalid
    assert lib.odh_dense_probe_gemm_verify(i8, pa, pb, 256, 256, 128, None, None, s) == invalid
    torch.cuda.synchronize(dev)
    assert int(c.abs().sum()) == 0 and int(counters.abs().sum()) == 0 and int(a.abs().sum()) == 0


# ------------------------------------------------------------------ fill and fused verify


def _model(fmt, m, n, k):
    """The operands ``odh_dense_fill`` writes, as int64."""
    a, bt = ref.probe_operands(m, n, k)
    return (a * I8_MUL_A, bt * I8_MUL_B) if fmt == "i8" else (a, bt)


def _table(fmt, k):
    return ref.probe_class_table(k) * (I8_MUL_A * I8_MUL_B if fmt == "i8" else 1)


def _filled(dev, fmt, m, n, k):
    gpu = _gpu()
    dtype = torch.int8 if fmt == "i8" else torch.float16
    a = torch.full((m, k), 77, dtype=dtype, device=dev)
    bt = torch.full((n, k), 77, dtype=dtype, device=dev)
    gpu.dense_fill(fmt, a, bt)
    return a, bt


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_fill_matches_the_model(dev, fmt):
    gpu = _gpu()
    assert (gpu.ODH_DT_I8_MUL_A, gpu.ODH_DT_I8_MUL_B) == (I8_MUL_A, I8_MUL_B)
    m, n, k = 256, 512, 192
    a, bt = _filled(dev, fmt, m, n, k)
    va, vb = _model(fmt, m, n, k)
    assert a.cpu().numpy().dtype == NP_DTYPE[fmt]
    assert np.array_equal(a.cpu().numpy().astype(np.int64), va)
    assert np.array_equal(bt.cpu().numpy().astype(np.int64), vb)
    # bit for bit: the halves are the model's, not merely equal in value (-0.0)
    assert np.array_equal(a.cpu().numpy().view(np.uint8), va.astype(NP_DTYPE[fmt]).view(np.uint8))
    assert np.array_equal(bt.cpu().numpy().view(np.uint8), vb.astype(NP_DTYPE[fmt]).view(np.uint8))


VERIFY_SHAPES = [(256, 256, s) for s in K_STAGES] + [(768, 768, None)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n,stages", VERIFY_SHAPES)
def test_dense_verify_clean(dev, fmt, m, n, stages):
    gpu = _gpu()
    k = 192 if stages is None else stages * _stage(fmt)
    assert k % 35 != 0
    r = gpu.dense_verify(fmt, *_filled(dev, fmt, m, n, k))
    assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert sum(r["xcd_blocks"]) == (m // 256) * (n // 256), r


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_verify_counts_a_corrupted_operand(dev, fmt):
    """One element of A replaced (copied in from a host tensor): the mismatches are the output
    elements at which the host product of the corrupted operands leaves the table."""
    gpu = _gpu()
    m, n, k = 512, 256, 192
    a, bt = _filled(dev, fmt, m, n, k)
    va, vb = _model(fmt, m, n, k)
    i, kk = 300, 77
    new = 100 if fmt == "i8" else 5
    assert va[i, kk] != new
    va[i, kk] = new
    a[i, kk:kk + 1].copy_(torch.tensor([new], dtype=a.dtype))
    wrong = (va @ vb.T) != _table(fmt, k)[np.arange(m)[:, None] % 5, np.arange(n)[None, :] % 7]
    want = int(wrong.sum())
    assert want == int((vb[:, kk] != 0).sum()) and 0 < want < n and not np.delete(wrong, i, axis=0).any()
    r = gpu.dense_verify(fmt, a, bt)
    assert r["errors"] == want and sum(r["err_xcd"]) == want, r
    assert sum(r["xcd_blocks"]) == 2, r


def test_dense_probe_reports_the_check(dev):
    for fmt in FORMATS:
        r = _gpu().dense_probe(0, fmt, 512, 512, 192)
        assert set(r) == {"errors", "err_xcd", "xcd_blocks", "ms", "tflops"}
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == 4 and r["ms"] > 0


# ------------------------------------------------------------------ the program


def _check_formats_pass(block, names):
    assert list(block) == names
    for fmt in names:
        f = block[fmt]
        assert f["ok"] is True and f["errors"] == 0, block
        assert f["tflops"] > 50 and f["ms"] > 0 and f["host_ms"] > 0, block  # the matrix cores, not a stub


def test_dense_program_passes_on_the_mi355x():
    rc, res, r = _run_probe("--dtypes", "f16,i8")
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and "mx" not in res
    _check_formats_pass(res["dtypes"], FORMATS)
    d = res["results"][0]
    assert d["gemm_errors"] == 0 and d["hbm_errors"] == 0
    assert res["timings_ms"]["dtypes"] > 0
    assert len(json.dumps(res["dtypes"], separators=(",", ":"))) < 256
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
    print("dtypes:", json.dumps(res["dtypes"]), "gemm_ms:", d["gemm_ms"], "timings_ms:", json.dumps(res["timings_ms"]))


def test_dense_program_with_mx_stays_under_the_message_limit():
    rc, res, r = _run_probe("--mx", "fp8,fp4", "--dtypes", "f16,i8")
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"]
    _check_formats_pass(res["dtypes"], FORMATS)
    _check_formats_pass(res["mx"], ["fp8", "fp4"])
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
    # --rccl-mib adds its object on top (it needs 2+ GPUs to mean anything): its fields at their widest
    rccl = ',"rccl":{"ranks":8,"ok":false,"errors":18446744073709551615,"mib":128,"load_ms":99999.99,' \
           '"init_ms":99999.99,"allreduce_ms":99999.9999,"busbw_gbps":99999.9}'
    assert len(r.stdout.strip().splitlines()[-1]) + len(rccl) < 4096


def test_dense_program_fails_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--dtypes", "f16,i8", "--inject-fault", "dtypes")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    # A[0][0] becomes +1: row 0 is wrong exactly where Bt[j][0] = ((11 j) mod 7) - 3 is non-zero
    _, vb = ref.probe_operands(1, 4096, 1)
    want = int((vb[:, 0] != 0).sum())
    assert 0 < want < 4096
    assert res["ok"] is False
    for fmt in FORMATS:
        assert res["dtypes"][fmt]["ok"] is False and res["dtypes"][fmt]["errors"] == want, res["dtypes"]
    assert "GPU 0" in res["error"] and "f16" in res["error"] and "XCD" in res["error"], res["error"]
    d = res["results"][0]
    assert d["ok"] is True and d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
