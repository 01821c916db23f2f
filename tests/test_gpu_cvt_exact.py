"""The converter kernels on a real MI355X against the host model (``cvt_reference.py``):
``v_cvt_scalef32_pk_fp8_f32`` / ``_bf8_f32`` / ``_fp4_f32``, ``v_cvt_scalef32_2xpk16_fp6_f32`` / ``_bf6_f32`` and
``v_cvt_pk_bf16_f32`` through ``odh_cvt_encode``, ``odh_cvt_quantize``, ``odh_cvt_probe_verify`` and
``odh-gpu-probe --cvt``.

Everything is bit-exact: a converter's answer is a code, and the model names it.  Random inputs are drawn
as bit patterns with an exponent field in 1 … 254, so they are normal finite f32 by generation and
nothing is filtered afterwards; the sweep over all 65536 high halves keeps every pattern, NaN,
infinities and subnormals included.  The tests corrupt data only; every pointer handed to a kernel
comes from a torch allocation of exactly the size the shape implies.
"""

import functools

import numpy as np
import pytest

import cvt_reference as cr
import mx_reference as mx
from probe_gpu import _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = list(cr.NAMES)
SCALED = [n for n in FORMATS if n != "bf16"]


def _codes(name, t):
    """A result of ``cvt_encode`` / ``mx_quantize`` as one code per element, sign included."""
    if name == "bf16":
        return t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64)
    return mx.unpack(cr.NAMES[name], t.cpu().numpy()).astype(np.int64)


def _assert_codes(what, got, want, x):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        xb = np.ascontiguousarray(x).reshape(-1).view(np.uint32)
        first = [(hex(int(xb[i])), hex(int(got.reshape(-1)[i])), hex(int(want.reshape(-1)[i]))) for i in bad[:8]]
        pytest.fail(f"{what}: {len(bad)} of {got.size} codes differ; (x bits, got, want) {first}")


@functools.lru_cache(maxsize=None)
def _family(name):
    return cr.family(cr.NAMES[name])


def _normal_bits(rng, n):
    """Seeded f32 bit patterns, normal and finite by generation: exponent field 1 … 254."""
    bits = (rng.integers(0, 2, n, dtype=np.uint32) << 31) | (rng.integers(1, 255, n, dtype=np.uint32) << 23) \
        | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    x = bits.view(np.float32)
    assert np.isfinite(x).all() and (np.abs(x) >= np.finfo(np.float32).tiny).all()  # nothing to filter
    return x


# ------------------------------------------------------------------ the bare instruction


@pytest.mark.parametrize("name", FORMATS)
def test_encode_of_the_whole_family(dev, name):
    """Every case of the fused check's family through the row kernel: 32 consecutive cases share a scale."""
    f = _family(name)
    n = len(f["x"])
    x = torch.from_numpy(f["x"].copy()).reshape(n // 32, 32).to(dev)
    assert (f["scale"].reshape(-1, 32) == f["scale"][::32, None]).all()
    sc = None if name == "bf16" else torch.from_numpy(f["scale"][::32].copy()).reshape(-1, 1).to(dev)
    _assert_codes(f"{name} family", _codes(name, _gpu().cvt_encode(name, x, sc)).reshape(-1), f["expect"], f["x"])


@pytest.mark.parametrize("name", SCALED)
def test_encode_of_every_high_half_at_five_scales(dev, name):
    """All 65536 f32 whose low 16 bits are zero (every sign, exponent and the top seven mantissa bits: NaN,
    infinities and subnormals included; none left out) at the smallest, the largest and the middle scales."""
    x = (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)
    tx = torch.from_numpy(x.copy()).reshape(-1, 32).to(dev)
    for byte in (1, 126, 127, 128, 254):
        sc = torch.full((tx.shape[0], 1), byte, dtype=torch.uint8, device=dev)
        with np.errstate(over="ignore", invalid="ignore"):
            want = cr.encode(cr.NAMES[name], x, byte)
        assert want.shape == (65536,)
        _assert_codes(f"{name} scale byte {byte}", _codes(name, _gpu().cvt_encode(name, tx, sc)).reshape(-1), want, x)


@pytest.mark.parametrize("name", SCALED)
def test_encode_of_random_normal_f32_at_random_scales(dev, name):
    rng = np.random.default_rng(4100 + cr.NAMES[name])
    n = 1 << 20
    x = _normal_bits(rng, n)
    sc = rng.integers(1, 255, size=(n // 32, 1), dtype=np.uint8)
    with np.errstate(over="ignore"):
        want = cr.encode(cr.NAMES[name], x, np.repeat(sc[:, 0], 32))
    got = _gpu().cvt_encode(name, torch.from_numpy(x.copy()).reshape(-1, 32).to(dev), torch.from_numpy(sc).to(dev))
    _assert_codes(f"{name} random", _codes(name, got).reshape(-1), want, x)
    finite = want & ~(1 << cr.sign_bit(cr.NAMES[name])) <= cr.CMAX[cr.NAMES[name]]
    assert 0.05 < finite.mean()  # not all overflow: a share of the draws lands in the format's range


def test_encode_bf16_of_random_normal_f32(dev):
    x = _normal_bits(np.random.default_rng(1616), 1 << 22)
    got = _gpu().cvt_encode("bf16", torch.from_numpy(x.copy()).reshape(-1, 1024).to(dev))
    assert got.dtype == torch.bfloat16
    _assert_codes("bf16 random", _codes("bf16", got).reshape(-1), cr.encode(cr.BF16, x), x)


# ------------------------------------------------------------------ the quantiser


SHAPES = [(1, 32), (3, 96), (5, 160), (257, 32), (256, 1024)]


@functools.lru_cache(maxsize=None)
def _quantiser_input(rows, k):
    """Seeded values over 40 binades, with all-zero blocks, blocks of one non-zero, blocks whose largest
    element lies beyond the overflow midpoint at the block's scale (1.99 · 2^n), and negative zeros."""
    rng = np.random.default_rng(1000 * rows + k)
    nb = rows * k // 32
    x = (rng.standard_normal((nb, 32)) * 2.0 ** rng.integers(-20, 20, size=(nb, 1))
         * 2.0 ** -rng.integers(0, 6, size=(nb, 32))).astype(np.float32)
    kind = np.arange(nb) % 5 if nb >= 5 else np.array([2] * nb)
    x[kind == 0] = 0
    one = np.flatnonzero(kind == 1)
    x[one] = 0
    x[one, one % 32] = -(2.0 ** (one % 30 - 15))
    sat = np.flatnonzero(kind == 2)
    top = 2.0 ** (sat % 24 - 12)
    x[sat] = rng.uniform(-1, 1, size=(len(sat), 32)) * top[:, None]  # below 2^n, and one element 1.99 · 2^n
    x[sat, (sat * 7) % 32] = 1.99 * top * np.where(sat & 1, -1, 1)
    x[kind == 3, 5] = -0.0
    x = x.reshape(rows, k)
    assert np.isfinite(x).all()
    return x


@pytest.mark.parametrize("name", FORMATS)
@pytest.mark.parametrize("rows,k", SHAPES)
def test_quantize_is_the_models(dev, name, rows, k):
    x = _quantiser_input(rows, k)
    codes, scales = _gpu().mx_quantize(name, torch.from_numpy(x).to(dev))
    want_codes, want_scales = cr.quantize(cr.NAMES[name], x)
    if name == "bf16":
        assert scales is None and codes.dtype == torch.bfloat16 and tuple(codes.shape) == (rows, k)
        _assert_codes(f"bf16 {rows}x{k}", _codes(name, codes), want_codes.astype(np.int64), x)
        return
    assert codes.dtype == scales.dtype == torch.uint8
    assert tuple(codes.shape) == (rows, _gpu().mx_row_bytes(name, k)) and tuple(scales.shape) == (rows, k // 32)
    assert np.array_equal(scales.cpu().numpy(), want_scales), f"{name} {rows}x{k} scales"
    assert np.array_equal(codes.cpu().numpy(), want_codes), f"{name} {rows}x{k} codes, byte for byte"
    if rows * k >= 160:  # the cases the input was built for are there
        assert (want_scales == 127).any() and (np.abs(mx.decode(cr.NAMES[name], want_codes)).max()
                                               == cr.magnitudes(cr.NAMES[name])[-1])
    # with the quantiser's own scales the bare instruction differs exactly where the model saturated
    raw = _gpu().cvt_encode(name, torch.from_numpy(x).to(dev), scales)
    want_raw = cr.encode(cr.NAMES[name], x, np.repeat(want_scales, 32, axis=1))
    _assert_codes(f"{name} {rows}x{k} raw", _codes(name, raw), want_raw, x)


@pytest.mark.parametrize("name", SCALED)
def test_quantized_operands_feed_the_matrix_cores(dev, name):
    """Quantise A and Bt on the GPU and hand the result to ``mx_gemm`` as it is: the product is the host
    product of the host-quantised operands, so the layout is the one the matrix cores read.  The values are
    small integers times a power of two per block, every block holding a 3: the quantisation is lossless and
    every partial sum an integer far below 2^24 quanta, so fp32 accumulation is exact in any order."""
    fmt = cr.NAMES[name]
    rng = np.random.default_rng(900 + fmt)
    m = n = 256
    k = 128

    def operand(rows):
        v = rng.integers(-3, 4, size=(rows, k)).astype(np.float64)
        v[:, ::32] = 3 * np.where(rng.random((rows, k // 32)) < 0.5, -1, 1)
        return (v * 2.0 ** np.repeat(rng.integers(0, 4, size=(rows, k // 32)), 32, axis=1)).astype(np.float32)

    a, bt = operand(m), operand(n)
    ha, hsa = cr.quantize(fmt, a)
    hb, hsb = cr.quantize(fmt, bt)
    assert np.array_equal(mx.scaled(fmt, ha, hsa), a) and np.array_equal(mx.scaled(fmt, hb, hsb), bt)
    want = mx.product(fmt, ha, hb, hsa, hsb)
    assert (np.abs(a.astype(np.float64)) @ np.abs(bt.astype(np.float64)).T).max() < 2 ** 24
    gpu = _gpu()
    qa, sa = gpu.mx_quantize(name, torch.from_numpy(a).to(dev))
    qb, sb = gpu.mx_quantize(name, torch.from_numpy(bt).to(dev))
    c = gpu.mx_gemm(name, qa, qb, sa, sb)
    assert np.array_equal(c.cpu().numpy().astype(np.float64), want)
    assert np.array_equal(want, a.astype(np.float64) @ bt.astype(np.float64).T)


def test_entry_points_check_before_launch(dev):
    gpu = _gpu()
    x = torch.zeros((4, 64), device=dev)
    s = torch.full((4, 2), 127, dtype=torch.uint8, device=dev)
    for bad in ("f16", "i8", 6, -1):
        with pytest.raises(ValueError):
            gpu.mx_quantize(bad, x)
    for bad_x in (x.double(), x.cpu(), x[:, :48], x.t(), x[:, :16].contiguous(), x.reshape(-1), x.reshape(2, 2, 64),
                  torch.zeros((4, 68), device=dev)[:, 4:]):
        with pytest.raises(ValueError):
            gpu.mx_quantize("fp8", bad_x)
        with pytest.raises(ValueError):
            gpu.cvt_encode("fp4", bad_x, s)
    flat = torch.zeros(4 * 64 + 4, device=dev)
    with pytest.raises(ValueError, match="aligned"):
        gpu.mx_quantize("fp6", flat[1:257].reshape(4, 64))  # contiguous, 4 bytes off
    for bad_s in (s.to(torch.int8), s.cpu(), s[:, :1].contiguous(), s.t().contiguous().t(), None):
        with pytest.raises(ValueError):
            gpu.cvt_encode("fp8", x, bad_s)
    with pytest.raises(ValueError):
        gpu.cvt_encode("bf16", x, s)
    table = torch.zeros(gpu.ODH_CVT_TABLE, dtype=torch.uint8, device=dev)
    for fn in (gpu.cvt_fill, gpu.cvt_verify):
        for bad_t in (table[:255], table.to(torch.int8), table.cpu()):
            with pytest.raises(ValueError):
                fn("fp8", bad_t)
        with pytest.raises(ValueError):
            fn("f16", table)
    lib = gpu.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    out = torch.zeros((4, 64), dtype=torch.uint8, device=dev)
    counters = torch.zeros(gpu.ODH_NCOUNT, dtype=torch.int32, device=dev)
    px, ps, po = x.data_ptr(), s.data_ptr(), out.data_ptr()
    invalid = 1  # hipErrorInvalidValue
    for args in ((6, px, ps, po, 4, 64), (0, px, ps, po, 0, 64), (0, px, ps, po, 4, 48), (0, px, ps, po, 4, 0),
                 (0, None, ps, po, 4, 64), (0, px, None, po, 4, 64), (0, px, ps, None, 4, 64), (0, px + 4, ps, po, 4, 64),
                 (0, px, ps, po + 4, 4, 64)):
        assert lib.odh_cvt_encode(*args, st) == invalid, args
        fmt, ax, asc, ao, r, kk = args
        assert lib.odh_cvt_quantize(fmt, ax, ao, asc, r, kk, st) == invalid, args
    assert lib.odh_cvt_fill(6, table.data_ptr(), st) == invalid and lib.odh_cvt_fill(0, None, st) == invalid
    assert lib.odh_cvt_probe_verify(6, table.data_ptr(), counters.data_ptr(), st) == invalid
    assert lib.odh_cvt_probe_verify(0, None, counters.data_ptr(), st) == invalid
    assert lib.odh_cvt_probe_verify(0, table.data_ptr(), None, st) == invalid
    torch.cuda.synchronize(dev)
    assert not out.any() and not counters.any() and not table.any()


# ------------------------------------------------------------------ the fused check


@pytest.mark.parametrize("name", FORMATS)
def test_fused_check_clean_and_with_one_table_byte_off(dev, name):
    gpu = _gpu()
    table = torch.full((gpu.ODH_CVT_TABLE,), 0xEE, dtype=torch.uint8, device=dev)
    gpu.cvt_fill(name, table)
    h = table.cpu().numpy()
    if name == "bf16":
        want = np.arange(1, 255)
    else:
        lo, hi = cr.scale_range(cr.NAMES[name])
        want = np.arange(lo + 127, hi + 128)
    assert np.array_equal(h[:len(want)], want) and not h[len(want):].any()
    r = gpu.cvt_verify(name, table)
    assert set(r) == {"errors", "err_xcd", "xcd_blocks", "ms", "gcvt_s"}
    assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert sum(r["xcd_blocks"]) == gpu.ODH_CVT_BLOCKS == 256 and all(b > 0 for b in r["xcd_blocks"]), r
    assert r["ms"] > 0 and r["gcvt_s"] > 0
    for at in (0, len(want) // 2, len(want) - 1):  # the first, a middle and the last scale
        table[at] += 1
        bad = gpu.cvt_verify(name, table)
        table[at] -= 1
        assert bad["errors"] > 0 and all(e > 0 for e in bad["err_xcd"]), (at, bad)
        assert sum(bad["err_xcd"]) == bad["errors"] and sum(bad["xcd_blocks"]) == 256, (at, bad)
        # every wave of every workgroup meets the same cases: the count is a multiple of 1024
        assert bad["errors"] % (256 * 4) == 0, (at, bad)
    assert gpu.cvt_verify(name, table)["errors"] == 0  # everything put back
    again = gpu.cvt_probe(0, name)
    assert again["errors"] == 0 and sum(again["xcd_blocks"]) == 256


# ------------------------------------------------------------------ the program


ALL = "fp8,bf8,fp4,fp6,bf6,bf16"
KEYS_WITHOUT = ["ok", "devices", "shape", "hbm_mib", "results", "links", "setup_ms", "timings_ms"]


def test_cvt_program_passes_with_every_format():
    rc, res, r = _run_probe("--cvt", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["cvt"]) == FORMATS
    for f in res["cvt"].values():
        assert list(f) == ["ok", "errors", "ms", "gcvt_s"], f  # no host_ms: the verdict's size (probe_cli.cpp)
        assert f["ok"] is True and f["errors"] == 0 and f["ms"] > 0 and f["gcvt_s"] > 0, res["cvt"]
    assert list(res) == KEYS_WITHOUT[:6] + ["cvt"] + KEYS_WITHOUT[6:]
    t = list(res["timings_ms"])
    assert t.index("rccl") < t.index("cvt") < t.index("total") and res["timings_ms"]["cvt"] > 0
    print("verdict bytes:", len(r.stdout.strip().splitlines()[-1]), "cvt:", res["cvt"], res["timings_ms"])


def test_cvt_program_after_every_other_step_under_the_message_limit():
    rc, res, r = _run_probe("--mx", "fp8,fp4,bf8,fp6,bf6", "--dtypes", "f16,i8", "--fp", "f32,f64", "--sparse",
                            "bf16,f16,i8,fp8,bf8", "--cvt", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    keys = list(res)
    assert keys.index("mx") < keys.index("dtypes") < keys.index("fp") < keys.index("sparse") < keys.index("cvt")
    assert keys[-3:] == ["cvt", "setup_ms", "timings_ms"]
    for step in ("mx", "dtypes", "fp", "sparse"):  # the other steps' entries keep their keys
        for f in res[step].values():
            assert list(f) == ["ok", "errors", "ms", "tflops", "host_ms"], (step, f)
    line = r.stdout.strip().splitlines()[-1]
    print("verdict bytes:", len(line))
    assert len(line) < 4096


def test_cvt_program_without_the_step_is_what_it_was():
    rc, res, r = _run_probe()
    assert rc == 0 and res["ok"], r.stdout
    assert list(res) == KEYS_WITHOUT and "cvt" not in res["timings_ms"]
    assert list(res["timings_ms"]) == ["exec", "hip_init", "alloc_fill", "alloc", "code_load", "fill", "probe", "xgmi",
                                       "rccl", "total"]


def test_cvt_program_fails_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--cvt", ALL, "--inject-fault", "cvt")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    assert res["ok"] is False
    for name in FORMATS:
        assert res["cvt"][name]["ok"] is False and res["cvt"][name]["errors"] > 0, res["cvt"]
        assert res["cvt"][name]["errors"] % 1024 == 0
    # the first failing format, and every XCD: each one's SIMDs met the corrupted scale
    assert "GPU 0" in res["error"] and "fp8" in res["error"] and "conversion mismatches" in res["error"], res["error"]
    assert "on XCD 0,1,2,3,4,5,6,7" in res["error"] and "256/256" in res["error"], res["error"]
    d = res["results"][0]
    assert d["ok"] is True and d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
