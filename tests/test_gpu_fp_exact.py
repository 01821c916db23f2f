"""The FP32 / FP64 probe kernels on a real MI355X against a host product:
``v_mfma_f32_32x32x2_f32`` and ``v_mfma_f64_16x16x4_f64`` through ``odh_fp_gemm``, ``odh_fp_fill``,
``odh_fp_probe_gemm_verify`` and ``odh-gpu-probe --fp``.

Everything but one test is bit-exact.  Operands are integers; each case checks on the CPU that
``sum_k |a| |b|`` stays below ``2^24`` (f32) or ``2^53`` (f64), so every partial sum is an integer
the accumulator holds and the result is exact in any summation order.  The one-hot cases compare
single rounded products bit for bit.  The exception multiplies uniform reals in f32 and holds
every element to Higham's bound, which allows any summation order.  The tests corrupt data only;
every pointer handed to a kernel comes from a torch allocation at least as large as the shape
implies.
"""

import functools
import json

import numpy as np
import pytest

import fp_reference as fp
import probe_reference as ref
from probe_gpu import _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = fp.FORMATS
# random operands: integers of up to 7 (f32) resp. 21 (f64) bits, so products fill 13 resp. 41 bits
RANDOM_BELOW = {"f32": 64, "f64": 2 ** 20}


# ------------------------------------------------------------------ store kernel


@functools.lru_cache(maxsize=None)
def _random_case(fmt, m, n, k):
    """Seeded random integer operands, A and Bt drawn independently (so ``A != Btᵀ`` and no
    symmetry hides a transposed C write or a wrong row formula), and their exact int64 product."""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + len(fmt) + (64 if fmt == "f64" else 32))
    hi = RANDOM_BELOW[fmt]
    a = rng.integers(-hi, hi + 1, size=(m, k), dtype=np.int64)
    bt = rng.integers(-hi, hi + 1, size=(n, k), dtype=np.int64)
    want = a @ bt.T
    # exact in any summation order: every partial sum stays below the accumulator's exact range
    assert (np.abs(a) @ np.abs(bt).T).max() < fp.EXACT_BELOW[fmt]
    assert not np.array_equal(want[:min(m, n), :min(m, n)], want[:min(m, n), :min(m, n)].T)
    return a.astype(fp.NP_DTYPE[fmt]), bt.astype(fp.NP_DTYPE[fmt]), want


def _exact_store(dev, fmt, m, n, k):
    gpu = _gpu()
    a, bt, want = _random_case(fmt, m, n, k)
    c = torch.full((m, n), float("nan"), dtype=torch.from_numpy(a).dtype, device=dev)
    gpu.fp_gemm(fmt, torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev), out=c)
    got = c.cpu().numpy()
    assert got.dtype == fp.NP_DTYPE[fmt]
    want = want.astype(fp.NP_DTYPE[fmt])  # exact: below the type's integer range
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{fmt} {m}x{n}x{k}: {len(bad)} wrong elements in {len(np.unique(bad[:, 0]))} rows and "
                    f"{len(np.unique(bad[:, 1]))} columns, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


# fewer than, equal to and more than the three stages in flight and the four ring slots: ring
# fill, wrap and drain; then a long K of 64 stages
K_STAGES = [1, 2, 3, 4, 5, 7, 64]
# one stage; non-square grids whose workgroup counts exercise the XCD remap's remainders
GRIDS = [(512, 1024), (768, 768), (256, 2816)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stages", K_STAGES)
def test_fp_gemm_exact_over_k(dev, fmt, stages):
    _exact_store(dev, fmt, 256, 256, stages * fp.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", GRIDS)
def test_fp_gemm_exact_over_grids(dev, fmt, m, n):
    _exact_store(dev, fmt, m, n, fp.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_fp_gemm_exact_over_tiles_and_stages(dev, fmt):
    """2 × 3 (f32) or 2 × 6 (f64) tiles at 3 stages: operand addresses with a tile offset and ``kt > 0``."""
    _exact_store(dev, fmt, 512, 768, 3 * fp.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_fp_gemm_onehot_products_bit_for_bit(dev, fmt):
    """Every output is one product of two normal numbers with full, all-ones or single-bit
    mantissas, plus exact zeros: the instruction rounds it once, to nearest even."""
    a, bt, want = fp.onehot_case(fmt)
    c = _gpu().fp_gemm(fmt, torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev))
    got = c.cpu().numpy().view(fp.NP_BITS[fmt])
    wbits = want.view(fp.NP_BITS[fmt])
    if not np.array_equal(got, wbits):
        bad = np.argwhere(got != wbits)
        i, j = bad[0]
        pytest.fail(f"{fmt}: {len(bad)} products differ, first C[{i}][{j}] = {got[i, j]:#x}, expected {wbits[i, j]:#x}")


def test_f32_gemm_on_reals_within_highams_bound(dev):
    """Uniform [-1, 1) reals at K = 1024 against the fp64 host product: every element within
    ``gamma_K (|A| |B|ᵀ)`` with ``gamma_K = K u / (1 - K u)``, ``u = 2^-24`` (Higham, Accuracy and
    Stability of Numerical Algorithms, (3.5)); it holds for any summation order, so it allows the
    kernel's k permutation."""
    m = n = 256
    k = 1024
    rng = np.random.default_rng(32001024)
    a = rng.uniform(-1.0, 1.0, size=(m, k)).astype(np.float32)
    bt = rng.uniform(-1.0, 1.0, size=(n, k)).astype(np.float32)
    a64, b64 = a.astype(np.float64), bt.astype(np.float64)
    want = a64 @ b64.T
    u = 2.0 ** -24
    bound = k * u / (1 - k * u) * (np.abs(a64) @ np.abs(b64).T)
    got = _gpu().fp_gemm("f32", torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev)).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"f32 reals: max error {err.max():.3e}, max error / bound {np.max(err / bound):.4f}")
    assert np.isfinite(got).all() and (err <= bound).all(), np.argwhere(err > bound)[:8].tolist()
    assert err.max() > 0  # f32 arithmetic, not a wider accumulator copied down


# ------------------------------------------------------------------ entry points refuse


@pytest.mark.parametrize("fmt", FORMATS)
def test_fp_entry_points_check_before_launch(dev, fmt):
    gpu = _gpu()
    k = 2 * fp.STAGE[fmt]
    a, bt, _ = _random_case(fmt, 256, 256, k)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev)
    good = ta.dtype
    other = torch.float32 if fmt == "f64" else torch.float64
    for fn in (gpu.fp_gemm, gpu.fp_verify, gpu.fp_fill):
        for bad in ("f16", "bf16", 1, 2):
            with pytest.raises(ValueError):
                fn(bad, ta, tb)
        with pytest.raises(TypeError):
            fn(fmt, ta.to(other), tb)
        with pytest.raises(TypeError):
            fn(fmt, ta, tb.to(torch.float16))
        with pytest.raises(TypeError):
            fn(fmt, ta.to(other), tb.to(other))  # the other format's dtype under this format's name
        with pytest.raises(ValueError):
            fn(fmt, ta.t(), tb)  # not contiguous
        with pytest.raises(ValueError):
            fn(fmt, ta[:, ::2], tb[:, ::2])  # not contiguous
        with pytest.raises(ValueError):
            fn(fmt, ta[:, :k // 4].contiguous(), tb[:, :k // 4].contiguous())  # K is half a stage
        with pytest.raises(ValueError):
            fn(fmt, ta[:128].contiguous(), tb)  # M = 128
        with pytest.raises(ValueError):
            fn(fmt, ta, tb[:128].contiguous())  # N = 128: a whole f64 tile, but N is a multiple of 256
        with pytest.raises(ValueError):
            fn(fmt, ta, tb[:, :k // 2].contiguous())  # K of A and of Bt differ
        with pytest.raises(ValueError):
            fn(fmt, ta.cpu(), tb)  # not on the same device
        with pytest.raises(ValueError):
            fn(fmt, ta[0], tb)  # not 2-D
        with pytest.raises(ValueError):
            fn(fmt, ta.flatten()[1:1 + 256 * k // 2].view(256, k // 2), tb[:, :k // 2].contiguous())  # 16-byte alignment
    # the probe's own operands are not exact past this K; any operands may be multiplied there
    big = 2736 if fmt == "f32" else 1368
    za = torch.zeros((256, big), dtype=good, device=dev)
    assert gpu.fp_shape_ok(fmt, 256, 256, big) and not gpu.fp_k_exact(fmt, big)
    for fn in (gpu.fp_fill, gpu.fp_verify):
        with pytest.raises(ValueError):
            fn(fmt, za, za)
    with pytest.raises(ValueError):
        gpu.fp_probe(0, fmt, 256, 256, big)
    with pytest.raises(ValueError):
        gpu.fp_probe(0, fmt, 256, 128, k)
    assert int(za.abs().sum()) == 0
    for out in (torch.empty((256, 256), dtype=other, device=dev), torch.empty((256, 128), dtype=good, device=dev),
                torch.empty((256, 256), dtype=good), torch.empty((256, 512), dtype=good, device=dev)[:, ::2]):
        with pytest.raises(ValueError):
            gpu.fp_gemm(fmt, ta, tb, out=out)


def test_fp_c_abi_refuses_before_launch(dev):
    """The library's own checks, below the Python ones: ``hipErrorInvalidValue`` and no launch.
    The buffers are large enough for every shape tried here."""
    gpu = _gpu()
    lib = gpu.load_library()
    invalid = 1  # hipErrorInvalidValue
    a = torch.zeros((512, 2736), dtype=torch.float64, device=dev)
    bt = torch.zeros((512, 2736), dtype=torch.float64, device=dev)
    c = torch.zeros((512, 512), dtype=torch.float64, device=dev)
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pa, pb, pc, pk = a.data_ptr(), bt.data_ptr(), c.data_ptr(), counters.data_ptr()
    f32, f64 = gpu.ODH_FP_F32, gpu.ODH_FP_F64
    for args in ((0, pa, pb, pc, 256, 256, 128), (1, pa, pb, pc, 256, 256, 128), (2, pa, pb, pc, 256, 256, 128),
                 (16, pa, pb, pc, 256, 256, 128), (-4, pa, pb, pc, 256, 256, 128),  # unknown formats
                 (f32, pa, pb, pc, 128, 256, 128), (f64, pa, pb, pc, 256, 384, 128), (f64, pa, pb, pc, 256, 128, 128),
                 (f32, pa, pb, pc, 256, 256, 8), (f64, pa, pb, pc, 256, 256, 4), (f64, pa, pb, pc, 256, 256, 12),
                 (f32, pa, pb, pc, 256, 256, 0), (f32, pa, pb, pc, 256, 256, -16), (f64, pa, pb, pc, 0, 256, 8),
                 (f64, None, pb, pc, 256, 256, 128), (f32, pa, None, pc, 256, 256, 128),
                 (f64, pa + 8, pb, pc, 256, 256, 64), (f32, pa, pb + 4, pc, 256, 256, 64)):  # not 16-byte aligned
        fmt, xa, xb, xc, m, n, k = args
        assert lib.odh_fp_gemm(fmt, xa, xb, xc, m, n, k, s) == invalid, args
        assert lib.odh_fp_fill(fmt, xa, xb, m, n, k, s) == invalid, args
        assert lib.odh_fp_probe_gemm_verify(fmt, xa, xb, m, n, k, None, pk, s) == invalid, args
    assert lib.odh_fp_gemm(f64, pa, pb, None, 256, 256, 128, s) == invalid
    assert lib.odh_fp_gemm(f64, pa, pb, pc + 4, 256, 256, 128, s) == invalid  # C not aligned to its element
    assert lib.odh_fp_probe_gemm_verify(f64, pa, pb, 256, 256, 128, None, None, s) == invalid
    # a K at which the probe operands' sums are no longer exact integers: fill and check refuse
    for fmt, k in ((f32, 2736), (f64, 1368)):
        assert lib.odh_fp_fill(fmt, pa, pb, 256, 256, k, s) == invalid, (fmt, k)
        assert lib.odh_fp_probe_gemm_verify(fmt, pa, pb, 256, 256, k, None, pk, s) == invalid, (fmt, k)
    for fmt, m, n, want in ((f32, 512, 768, 6), (f64, 512, 768, 12), (f64, 4096, 4096, 512), (f32, 4096, 4096, 256),
                            (f32, 128, 256, 0), (f64, 256, 128, 0), (0, 256, 256, 0), (f64, 0, 256, 0)):
        assert lib.odh_fp_tiles(fmt, m, n) == want, (fmt, m, n)
    torch.cuda.synchronize(dev)
    assert int(c.abs().sum()) == 0 and int(counters.abs().sum()) == 0 and int(a.abs().sum()) == 0
    assert int(bt.abs().sum()) == 0


# ------------------------------------------------------------------ fill and fused verify


def _filled(dev, fmt, m, n, k):
    gpu = _gpu()
    dtype = torch.float64 if fmt == "f64" else torch.float32
    a = torch.full((m, k), 77, dtype=dtype, device=dev)
    bt = torch.full((n, k), 77, dtype=dtype, device=dev)
    gpu.fp_fill(fmt, a, bt)
    return a, bt


@pytest.mark.parametrize("fmt", FORMATS)
def test_fp_fill_matches_the_model(dev, fmt):
    gpu = _gpu()
    assert (gpu.ODH_FP_F32_MUL_A, gpu.ODH_FP_F32_MUL_B) == fp.MUL["f32"]
    assert (gpu.ODH_FP_F64_MUL_A, gpu.ODH_FP_F64_MUL_B) == fp.MUL["f64"]
    m, n, k = 256, 512, 192
    a, bt = _filled(dev, fmt, m, n, k)
    va, vb = fp.operands(fmt, m, n, k)
    assert a.cpu().numpy().dtype == fp.NP_DTYPE[fmt]
    # bit for bit: the floats are the model's, not merely equal in value (-0.0)
    assert np.array_equal(a.cpu().numpy().view(np.uint8), va.view(np.uint8))
    assert np.array_equal(bt.cpu().numpy().view(np.uint8), vb.view(np.uint8))


VERIFY_SHAPES = [(256, 256, s) for s in K_STAGES] + [(768, 768, None)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n,stages", VERIFY_SHAPES)
def test_fp_verify_clean(dev, fmt, m, n, stages):
    gpu = _gpu()
    k = 192 if stages is None else stages * fp.STAGE[fmt]
    assert k % 35 != 0 and fp.k_exact(fmt, k)
    r = gpu.fp_verify(fmt, *_filled(dev, fmt, m, n, k))
    assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert sum(r["xcd_blocks"]) == fp.tiles(fmt, m, n) == gpu.fp_tiles(fmt, m, n), r


@pytest.mark.parametrize("fmt", FORMATS)
def test_fp_verify_counts_a_corrupted_operand(dev, fmt):
    """One element of A replaced (copied in from a host tensor): the mismatches are the output
    elements at which the host product of the corrupted operands leaves the table."""
    gpu = _gpu()
    m, n, k = 512, 256, 192
    a, bt = _filled(dev, fmt, m, n, k)
    va, vb = fp.operand_values(fmt, m, n, k)
    i, kk = 300, 77
    new = 5 * fp.MUL[fmt][0]
    assert va[i, kk] != new
    va[i, kk] = new
    a[i, kk:kk + 1].copy_(torch.tensor([new], dtype=a.dtype))
    assert (np.abs(va) @ np.abs(vb).T).max() < fp.EXACT_BELOW[fmt]
    wrong = (va @ vb.T) != fp.expected(fmt, m, n, k)
    want = int(wrong.sum())
    assert want == int((vb[:, kk] != 0).sum()) and 0 < want < n and not np.delete(wrong, i, axis=0).any()
    r = gpu.fp_verify(fmt, a, bt)
    assert r["errors"] == want and sum(r["err_xcd"]) == want, r
    assert sum(r["xcd_blocks"]) == fp.tiles(fmt, m, n) == (2 if fmt == "f32" else 4), r


def test_fp_probe_reports_the_check(dev):
    for fmt in FORMATS:
        r = _gpu().fp_probe(0, fmt, 512, 512, 192)
        assert set(r) == {"errors", "err_xcd", "xcd_blocks", "ms", "tflops"}
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == fp.tiles(fmt, 512, 512) and r["ms"] > 0


# ------------------------------------------------------------------ the program


@functools.lru_cache(maxsize=None)
def _program_run():
    return _run_probe("--fp", "f32,f64")


def test_fp_program_passes_on_the_mi355x():
    rc, res, r = _program_run()
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and "mx" not in res and "dtypes" not in res
    assert list(res["fp"]) == FORMATS
    for fmt in FORMATS:
        f = res["fp"][fmt]
        assert f["ok"] is True and f["errors"] == 0 and f["ms"] > 0 and f["host_ms"] > 0, res["fp"]
    d = res["results"][0]
    assert d["gemm_errors"] == 0 and d["hbm_errors"] == 0
    assert res["timings_ms"]["fp"] > 0
    assert list(res)[-3:] == ["fp", "setup_ms", "timings_ms"]
    assert len(json.dumps(res["fp"], separators=(",", ":"))) < 256
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
    print("fp:", json.dumps(res["fp"]), "gemm_ms:", d["gemm_ms"], "timings_ms:", json.dumps(res["timings_ms"]))


def test_fp_program_f32_rate_is_the_matrix_cores():
    """The f32 MFMA rate is 1/16 of bf16's, and the bf16 kernel's fixed prologue and check are a
    16 times smaller share of the f32 run: within one verdict f32 reaches a sixteenth of bf16."""
    rc, res, r = _program_run()
    assert rc == 0, (r.stdout, r.stderr)
    f32, bf16 = res["fp"]["f32"]["tflops"], res["results"][0]["gemm_tflops"]
    print(f"f32 {f32} TFLOP/s, bf16 {bf16} TFLOP/s, bf16 / 16 = {bf16 / 16:.1f}; f64 {res['fp']['f64']}")
    assert f32 >= bf16 / 16
    assert res["fp"]["f64"]["ms"] > 0


def test_fp_program_with_every_step_stays_under_the_message_limit():
    rc, res, r = _run_probe("--mx", "fp8,fp4,bf8,fp6,bf6", "--dtypes", "f16,i8", "--fp", "f32,f64")
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"]
    assert list(res["mx"]) == ["fp8", "fp4", "bf8", "fp6", "bf6"] and list(res["dtypes"]) == ["f16", "i8"]
    assert list(res["fp"]) == FORMATS
    keys = list(res)
    assert keys.index("mx") < keys.index("dtypes") < keys.index("fp")
    t = list(res["timings_ms"])
    assert t.index("mx") < t.index("dtypes") < t.index("fp") < t.index("total")
    for step in ("mx", "dtypes", "fp"):
        for f in res[step].values():
            assert f["ok"] is True and f["errors"] == 0 and f["ms"] > 0, res[step]
    # --rccl-mib adds its object on top (it needs 2+ GPUs to mean anything): its fields at their widest
    rccl = ',"rccl":{"ranks":8,"ok":false,"errors":18446744073709551615,"mib":128,"load_ms":99999.99,' \
           '"init_ms":99999.99,"allreduce_ms":99999.9999,"busbw_gbps":99999.9}'
    assert len(r.stdout.strip().splitlines()[-1]) + len(rccl) < 4096


def test_fp_program_fails_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--fp", "f32,f64", "--inject-fault", "fp")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    # A[0][0] becomes +MUL_A: row 0 is wrong exactly where Bt[j][0] = ((11 j) mod 7) - 3 is non-zero
    _, vb = ref.probe_operands(1, 4096, 1)
    want = int((vb[:, 0] != 0).sum())
    assert 0 < want < 4096
    assert res["ok"] is False
    for fmt in FORMATS:
        assert res["fp"][fmt]["ok"] is False and res["fp"][fmt]["errors"] == want, res["fp"]
    assert "GPU 0" in res["error"] and "f32" in res["error"] and "XCD" in res["error"], res["error"]
    d = res["results"][0]
    assert d["ok"] is True and d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
