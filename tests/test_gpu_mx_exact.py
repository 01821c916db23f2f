"""The block-scaled probe kernels on a real MI355X against the host model (``mx_reference.py``):
``mx_gemm256_kernel`` (``gpu_probe_mx.h``, ``v_mfma_scale_f32_32x32x64_f8f6f4``) through
``odh_mx_gemm``, ``odh_mx_fill``, ``odh_mx_probe_gemm_verify`` and ``odh-gpu-probe --mx``.

Every test here is written for all five operand formats and runs on ``FORMATS``, FP8 and MXFP4.
``test_gpu_mx_formats_exact.py`` runs the same functions on BF8, FP6 and BF6 under the names
those cases have always had; the sweeps over every row, column, scale byte and code are in
``test_gpu_lowprec_sweeps.py``.

Everything is bit-exact.  Operands are small dyadic numbers and scales powers of two, so every
product is exact in fp32; each random case checks on the CPU that ``sum_k |a| |b|`` stays below
``2^24`` quanta, so every partial sum is representable and fp32 accumulation is exact in any
order.  The tests corrupt data only; every pointer handed to a kernel comes from a torch
allocation of exactly the size the shape implies.
"""

import functools
import json

import numpy as np
import pytest

import mx_reference as ref
from probe_gpu import _gpu, _mx_filled as _filled, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = ["fp8", "fp4"]
ALL_FIVE = ["fp8", "fp4", "bf8", "fp6", "bf6"]


def _stage(fmt):
    return 64 if fmt in ("fp8", "bf8") else 128  # elements per stage of a row: 64 bytes, or 96 of FP6 / BF6


# ------------------------------------------------------------------ store kernel

# every exactly representable value used: FP8 and BF8 the integers -8 .. 8, FP4 all 15 values, FP6
# the 31 multiples of 1/2 up to ±7.5, BF6 the multiples of 1/2 up to ±8 that e3m2 holds (steps of
# 1/2 to 4, of 1 to 8)
_BF6_HALVES = np.array([0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 5, 6, 7, 8])
VALUES = {"fp8": np.arange(-8, 9, dtype=np.float64),
          "fp4": np.concatenate([-ref.FP4_VALUES[:0:-1], ref.FP4_VALUES]),
          "bf8": np.arange(-8, 9, dtype=np.float64),
          "fp6": np.arange(-15, 16, dtype=np.float64) / 2,
          "bf6": np.concatenate([-_BF6_HALVES[::-1], [0.0], _BF6_HALVES])}
# the smallest product of two operands times two scales of 2^-2: the quantum of every sum
QUANTUM = {"fp8": 2.0 ** -4, "fp4": 2.0 ** -6, "bf8": 2.0 ** -4, "fp6": 2.0 ** -6, "bf6": 2.0 ** -6}

# 1, 2, 3 and 5 stages (both buffers, odd and even counts) and a long K: 64 stages, or 16 of FP6 /
# BF6 (K = 2048: at 64 stages the 6-bit value sets exceed the 2^24 bound)
K_STAGES = {fmt: [1, 2, 3, 5, 16 if fmt in ("fp6", "bf6") else 64] for fmt in ALL_FIVE}
# one stage; workgroup counts = 0, 1 and 7 mod 8 (the XCD remap's three cases), then a single
# tile row of 11
GRIDS = [(512, 1024), (768, 768), (1280, 768), (256, 2816)]
VERIFY_SHAPES = [(256, 256, 256), (512, 768, 384), (1280, 768, 1024)]


@functools.lru_cache(maxsize=None)
def _random_case(fmt, m, n, k):
    """Seeded codes over ``VALUES``, scales 2^-2 .. 2^2, and the float64 product of the decoded,
    scaled operands (decoded bit by bit by the model, not by the encoder that made the codes)."""
    code = ref.NAMES[fmt]
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + code)
    a = ref.encode(code, rng.choice(VALUES[fmt], size=(m, k)))
    bt = ref.encode(code, rng.choice(VALUES[fmt], size=(n, k)))
    row_bytes = _gpu().mx_row_bytes(fmt, k)
    assert a.shape == (m, row_bytes) and bt.shape == (n, row_bytes)
    sa = rng.integers(125, 130, size=(m, k // 32), dtype=np.uint8)
    sbt = rng.integers(125, 130, size=(n, k // 32), dtype=np.uint8)
    xa, xb = ref.scaled(code, a, sa), ref.scaled(code, bt, sbt)
    want = xa @ xb.T
    # exact in fp32 in any summation order: every partial sum is a multiple of the quantum
    # below 2^24 quanta (and float64 holds them with 29 bits to spare)
    assert (np.abs(xa) @ np.abs(xb).T).max() < 2.0 ** 24 * QUANTUM[fmt]
    return a, bt, sa, sbt, want


def _exact_store(dev, fmt, m, n, k):
    gpu = _gpu()
    a, bt, sa, sbt, want = _random_case(fmt, m, n, k)
    c = torch.full((m, n), float("nan"), device=dev)
    t = [torch.from_numpy(x).to(dev) for x in (a, bt, sa, sbt)]
    gpu.mx_gemm(fmt, *t, out=c)
    got = c.cpu().double().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{fmt} {m}x{n}x{k}: {len(bad)} wrong elements, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stages", K_STAGES["fp8"])
def test_mx_gemm_exact_over_k(dev, fmt, stages):
    _exact_store(dev, fmt, 256, 256, stages * _stage(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", GRIDS)
def test_mx_gemm_exact_over_grids(dev, fmt, m, n):
    _exact_store(dev, fmt, m, n, _stage(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_gemm_exact_over_tiles_and_stages(dev, fmt):
    """2 × 3 tiles at 3 stages: operand and scale addresses with a tile offset and ``kt > 0``."""
    _exact_store(dev, fmt, 512, 768, 3 * _stage(fmt))


def test_mx_entry_points_check_before_launch(dev):
    gpu = _gpu()
    a, bt, sa, sbt, _ = _random_case("fp8", 256, 256, 64)
    t = [torch.from_numpy(x).to(dev) for x in (a, bt, sa, sbt)]
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp6", *t)
    with pytest.raises(TypeError):
        gpu.mx_gemm("fp8", t[0].to(torch.int8), *t[1:])
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp8", t[0].cpu(), *t[1:])
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp8", t[0].t(), *t[1:])
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp4", *t)  # 64 bytes per row are 128 FP4 elements: the scales are [256, 4]
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp8", t[0][:128].contiguous(), *t[1:])
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp8", *t[:3], t[3][:, :1].contiguous())


# ------------------------------------------------------------------ fill


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_fill_matches_the_model(dev, fmt):
    m, n, k = 256, 256, 384
    a, bt, sa, sbt, table = _filled(dev, fmt, m, n, k)
    va, vb = ref.probe_values(m, n, k)
    code = ref.NAMES[fmt]
    assert np.array_equal(a.cpu().numpy(), ref.encode(code, va))
    assert np.array_equal(bt.cpu().numpy(), ref.encode(code, vb))
    assert np.array_equal(ref.decode(code, a.cpu().numpy()), va)
    assert np.array_equal(ref.decode(code, bt.cpu().numpy()), vb)
    assert np.array_equal(sa.cpu().numpy(), ref.probe_scales(m, k))
    assert np.array_equal(sbt.cpu().numpy(), ref.probe_scales(n, k))
    t = ref.probe_table(k)
    assert np.array_equal(table.cpu().double().numpy(), t)
    # the table is the product of the operands as filled: the closed form holds
    want = ref.product(code, a.cpu().numpy(), bt.cpu().numpy(), sa.cpu().numpy(), sbt.cpu().numpy())
    assert np.array_equal(want, t[np.arange(m)[:, None] % ref.ROWS, np.arange(n)[None, :] % ref.COLS])


# ------------------------------------------------------------------ fused verify

# byte 0 of A with A[0][0] = +3 (A[0][1] is 0, so the byte holds nothing else in FP4's high nibble or
# the packed formats' upper two bits)
THREE = {"fp8": 0x44, "fp4": 0x05, "bf8": 0x42, "fp6": 0x14, "bf6": 0x12}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n,k", VERIFY_SHAPES)
def test_mx_verify_clean(dev, fmt, m, n, k):
    gpu = _gpu()
    assert ref.zero_classes(k) == 0
    r = gpu.mx_verify(fmt, *_filled(dev, fmt, m, n, k))
    assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert sum(r["xcd_blocks"]) == (m // 256) * (n // 256), r


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_verify_finds_a_corrupted_operand(dev, fmt):
    """``A[0][0]`` becomes +3 as ``--inject-fault mx`` makes it, by writing byte 0: row 0 is wrong
    exactly where ``Bt[j][0] = ((11 j) mod 7) - 3`` is non-zero."""
    gpu = _gpu()
    m, n, k = 256, 256, 256
    a, bt, sa, sbt, table = _filled(dev, fmt, m, n, k)
    host = a[:1].cpu().numpy()
    assert ref.decode(ref.NAMES[fmt], host)[0, :2].tolist() == [-2.0, 0.0]
    host[0, 0] = THREE[fmt]
    assert ref.decode(ref.NAMES[fmt], host)[0, :2].tolist() == [3.0, 0.0]
    a[0, 0] = THREE[fmt]
    want = sum(1 for j in range(n) if (11 * j) % 7 != 3)
    assert want == 220
    r = gpu.mx_verify(fmt, a, bt, sa, sbt, table)
    assert r["errors"] == want and sum(r["err_xcd"]) == want, r
    assert sum(1 for x in r["err_xcd"] if x) == 1, r  # one tile, so one XCD


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_verify_reads_each_blocks_scale(dev, fmt):
    """Scale byte ``sA[0][0]`` goes from 126 to 130: only the first 32 k of row 0 change weight,
    and the mismatches are the columns where the model's row 0 then differs from the table."""
    gpu = _gpu()
    m, n, k = 256, 256, 256
    a, bt, sa, sbt, table = _filled(dev, fmt, m, n, k)
    assert int(sa[0, 0]) == 126
    sa[0, 0] = 130
    code = ref.NAMES[fmt]
    row = ref.product(code, a[:1].cpu().numpy(), bt.cpu().numpy(), sa[:1].cpu().numpy(), sbt.cpu().numpy())[0]
    want = int((row != ref.probe_table(k)[0, np.arange(n) % ref.COLS]).sum())
    assert 0 < want < n
    r = gpu.mx_verify(fmt, a, bt, sa, sbt, table)
    assert r["errors"] == want and sum(r["err_xcd"]) == want, r


def test_mx_probe_reports_the_check(dev, formats=FORMATS):
    for fmt in formats:
        r = _gpu().mx_probe(0, fmt, 512, 512, 256)
        assert set(r) >= {"errors", "err_xcd", "xcd_blocks", "ms", "tflops"}
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == 4 and r["ms"] > 0, (fmt, r)


# ------------------------------------------------------------------ the program


def _program_passes(formats, *more):
    """``odh-gpu-probe --mx formats`` (and ``more`` arguments) passes, one entry per format in the
    order given, each from the matrix cores.  Returns the verdict and its line."""
    rc, res, r = _run_probe("--mx", ",".join(formats), *more)
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["mx"]) == formats
    for fmt in formats:
        f = res["mx"][fmt]
        assert f["ok"] is True and f["errors"] == 0, res["mx"]
        assert f["tflops"] > 50 and f["ms"] > 0 and f["host_ms"] > 0, res["mx"]  # the matrix cores, not a stub
    d = res["results"][0]
    assert d["gemm_errors"] == 0 and d["hbm_errors"] == 0
    line = r.stdout.strip().splitlines()[-1]
    assert len(line.encode()) < 4096, len(line.encode())
    print("verdict bytes:", len(line.encode()), "mx:", json.dumps(res["mx"]), "timings_ms:", json.dumps(res["timings_ms"]))
    return res, line


def _program_fails_on_injected_fault(formats, n, *more):
    """``--inject-fault mx`` at N = ``n``: every format counts the columns of row 0 where
    ``Bt[j][0]`` is non-zero, and the bf16 checks stay clean."""
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--mx", ",".join(formats), *more, "--inject-fault", "mx")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    want = sum(1 for j in range(n) if (11 * j) % 7 != 3)
    assert want == {4096: 3511, 256: 220}[n]
    assert res["ok"] is False and list(res["mx"]) == formats
    for fmt in formats:
        assert res["mx"][fmt]["ok"] is False and res["mx"][fmt]["errors"] == want, res["mx"]
    assert "GPU 0" in res["error"] and "fp8" in res["error"] and "XCD" in res["error"], res["error"]
    d = res["results"][0]
    assert d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1].encode()) < 4096


def test_mx_program_passes_on_the_mi355x():
    res, _ = _program_passes(FORMATS)
    assert len(json.dumps(res["mx"], separators=(",", ":"))) < 256


def test_mx_program_fails_on_injected_fault():
    _program_fails_on_injected_fault(FORMATS, 4096)
