"""The BF8 / FP6 / BF6 block-scaled probe kernels on a real MI355X against the host model
(``mx_formats_reference.py``): ``mx_gemm256_kernel<BF8>`` and ``mx6_gemm256_kernel<FP6|BF6>``
(``gpu_probe_mx.h``) through ``odh_mx_gemm``, ``odh_mx_fill``, ``odh_mx_probe_gemm_verify`` and
``odh-gpu-probe --mx fp8,fp4,bf8,fp6,bf6``.

Everything is bit-exact.  Operands are small dyadic numbers and scales powers of two, so every
product is exact in fp32; each random case checks on the CPU that ``sum_k |a| |b|`` stays below
``2^24`` quanta, so every partial sum is representable and fp32 accumulation is exact in any
order, and the one-hot cases have a single product per output.  The tests corrupt data only;
every pointer handed to a kernel comes from a torch allocation of exactly the size the shape
implies (a launch's counter row and tile map are rows of such an allocation).
"""

import faulthandler
import functools
import json
import os
import subprocess
import types

import numpy as np
import pytest

import mx_formats_reference as ref
import mx_reference as mx

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = ["bf8", "fp6", "bf6"]
PACKED = ["fp6", "bf6"]
ALL_FIVE = ["fp8", "fp4", "bf8", "fp6", "bf6"]
TEST_TIMEOUT_S = 60  # per test: a hung kernel ends the run here instead of holding the GPU


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(TEST_TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from odh_kubeflow_amd.ops import gpu

    gpu.load_library()  # loud failure if the in-tree .so is missing
    return torch.device("cuda", 0)


def _gpu():
    from odh_kubeflow_amd.ops import gpu

    return gpu


def _stage(fmt):
    return 64 if fmt == "bf8" else 128  # elements per stage of a row: 64 bytes of BF8, 96 of FP6 / BF6


def _row_bytes(fmt, k):
    return k if fmt == "bf8" else k // 4 * 3


# ------------------------------------------------------------------ store kernel, random codes

# BF8 the integers -8 .. 8, FP6 the 31 multiples of 1/2 up to ±7.5, BF6 the multiples of 1/2 up to
# ±8 that e3m2 holds (steps of 1/2 to 4, of 1 to 8)
_BF6_HALVES = np.array([0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 5, 6, 7, 8])
VALUES = {"bf8": np.arange(-8, 9, dtype=np.float64),
          "fp6": np.arange(-15, 16, dtype=np.float64) / 2,
          "bf6": np.concatenate([-_BF6_HALVES[::-1], [0.0], _BF6_HALVES])}
# the smallest product of two operands times two scales of 2^-2: the quantum of every sum
QUANTUM = {"bf8": 2.0 ** -4, "fp6": 2.0 ** -6, "bf6": 2.0 ** -6}


@functools.lru_cache(maxsize=None)
def _random_case(fmt, m, n, k):
    """Seeded codes over ``VALUES``, scales 2^-2 .. 2^2, and the float64 product of the decoded,
    scaled operands (decoded bit by bit by the model, not by the encoder that made the codes)."""
    code = ref.NAMES[fmt]
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + code)
    a = ref.encode(code, rng.choice(VALUES[fmt], size=(m, k)))
    bt = ref.encode(code, rng.choice(VALUES[fmt], size=(n, k)))
    assert a.shape == (m, _row_bytes(fmt, k)) and bt.shape == (n, _row_bytes(fmt, k))
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


# 1, 2, 3 and 5 stages (both buffers, odd and even counts) and a long K: 64 stages of BF8, 16 of
# FP6 / BF6 (K = 2048: at 64 stages the 6-bit value sets exceed the 2^24 bound)
K_STAGES = {"bf8": [1, 2, 3, 5, 64], "fp6": [1, 2, 3, 5, 16], "bf6": [1, 2, 3, 5, 16]}
# one stage; workgroup counts = 0, 1 and 7 mod 8 (the XCD remap's three cases), then a single
# tile row of 11
GRIDS = [(512, 1024), (768, 768), (1280, 768), (256, 2816)]


@pytest.mark.parametrize("fmt,stages", [(f, s) for f in FORMATS for s in K_STAGES[f]])
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


def test_mx_entry_points_check_the_new_layouts(dev):
    gpu = _gpu()
    a, bt, sa, sbt, _ = _random_case("fp6", 256, 256, 128)
    t = [torch.from_numpy(x).to(dev) for x in (a, bt, sa, sbt)]
    assert t[0].shape == (256, 96)
    assert tuple(gpu.mx_gemm("fp6", *t).shape) == (256, 256)  # the layout that is accepted
    with pytest.raises(ValueError):
        gpu.mx_gemm("bf8", *t)  # 96 bytes per row are no whole number of BF8 stages
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp6", t[0][:, :64].contiguous(), t[1][:, :64].contiguous(), *t[2:])  # rows of 64 bytes
    with pytest.raises(ValueError):
        gpu.mx_gemm("bf6", *t[:3], t[3][:, :2].contiguous())  # the scales are [256, 4]
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp5", *t)


# ------------------------------------------------------------------ store kernel: code against code


def _assert_store_exact(what, got, want):
    """NaN exactly where the model has NaN, equal by value elsewhere (so the same-signed infinity
    where the model has one; -0 equals 0).  ``got`` was pre-filled with 3e38, which no case
    expects, so an element never stored fails too."""
    got = got.astype(np.float64)
    nan = np.isnan(want)
    wrong = np.where(nan, ~np.isnan(got), got != want)
    if wrong.any():
        bad = np.argwhere(wrong)
        rows, cols = np.unique(bad[:, 0]), np.unique(bad[:, 1])
        for i, j in bad[:8]:
            print(f"{what}: C[{i}][{j}] = {got[i, j]!r}, expected {want[i, j]!r}")
        pytest.fail(f"{what}: {len(bad)} wrong elements in {len(rows)} rows "
                    f"{[hex(r) for r in rows[:40]]} and {len(cols)} columns {[hex(c) for c in cols[:40]]}")


def _mx_store(dev, fmt, case):
    a, bt, sa, sbt, want = case
    c = torch.full(want.shape, 3e38, device=dev)
    _gpu().mx_gemm(fmt, *[torch.from_numpy(x).to(dev) for x in (a, bt, sa, sbt)], out=c)
    return c.cpu().numpy(), want


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_store_decodes_every_code_against_every_code(dev, fmt):
    """BF8: all 256 × 256 pairs of codes (subnormals, ±57344, both infinities and the six NaN
    codes included); the expected value is the IEEE product of the model, and the MI355X agrees
    with it on the infinities too (inf · x = ±inf, inf · 0 = NaN), so no exception is listed.
    FP6 / BF6: all 64 × 64 pairs sixteen times over, at all 128 positions of a stage.  Seeded
    scales 2^-8 .. 2^8; each output is one product."""
    got, want = _mx_store(dev, fmt, ref.all_codes_case(ref.NAMES[fmt]))
    _assert_store_exact(f"{fmt} code i × code j", got, want)


def test_fp6_store_applies_every_scale_byte(dev):
    """E8M0 bytes 1 .. 254 through the FP6 kernel's own scale loads (one u32 per row and stage, 64
    stages): 1.0 · 1.0 under ``sA = i`` and an ``sBt`` that brings the pair back to 2^-20 .. 2^20."""
    got, want = _mx_store(dev, "fp6", ref.e8m0_range_case())
    _assert_store_exact("fp6 scale i", got, want)


# ------------------------------------------------------------------ fill


def _filled(dev, fmt, m, n, k):
    gpu = _gpu()
    rb = _row_bytes(fmt, k)
    a = torch.full((m, rb), 0xEE, dtype=torch.uint8, device=dev)
    bt = torch.full((n, rb), 0xEE, dtype=torch.uint8, device=dev)
    sa = torch.zeros((m, k // 32), dtype=torch.uint8, device=dev)
    sbt = torch.zeros((n, k // 32), dtype=torch.uint8, device=dev)
    table = torch.full(gpu.MX_TABLE, float("nan"), device=dev)
    gpu.mx_fill(fmt, a, bt, sa, sbt, table)
    return a, bt, sa, sbt, table


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
    assert np.array_equal(want, t[np.arange(m)[:, None] % mx.ROWS, np.arange(n)[None, :] % mx.COLS])


# ------------------------------------------------------------------ fused verify

THREE = {"bf8": 0x42, "fp6": 0x14, "bf6": 0x12}  # byte 0 of A with A[0][0] = +3 (A[0][1] is 0)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n,k", [(256, 256, 256), (512, 768, 384), (1280, 768, 1024)])
def test_mx_verify_clean(dev, fmt, m, n, k):
    gpu = _gpu()
    assert mx.zero_classes(k) == 0
    r = gpu.mx_verify(fmt, *_filled(dev, fmt, m, n, k))
    assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert sum(r["xcd_blocks"]) == (m // 256) * (n // 256), r


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_verify_finds_a_corrupted_operand(dev, fmt):
    """``A[0][0]`` becomes +3 as ``--inject-fault mx`` makes it, by writing byte 0 (``A[0][1]`` is 0,
    so the byte holds nothing else in the packed formats): row 0 is wrong exactly where
    ``Bt[j][0] = ((11 j) mod 7) - 3`` is non-zero."""
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
    want = int((row != ref.probe_table(k)[0, np.arange(n) % mx.COLS]).sum())
    assert 0 < want < n
    r = gpu.mx_verify(fmt, a, bt, sa, sbt, table)
    assert r["errors"] == want and sum(r["err_xcd"]) == want, r


def test_mx_probe_reports_the_check(dev):
    for fmt in FORMATS:
        r = _gpu().mx_probe(0, fmt, 512, 512, 256)
        assert set(r) >= {"errors", "err_xcd", "xcd_blocks", "ms", "tflops"}
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == 4 and r["ms"] > 0, (fmt, r)


# ------------------------------------------------------------------ fused verify: every row and column

SWEEP_SHAPE = (512, 512, 384)  # 2 × 2 tiles; 6 stages of BF8, 3 of FP6 / BF6; no class expecting 0


@functools.lru_cache(maxsize=None)
def _probe(fmt):
    """The probe operands of ``fmt`` on the GPU (written by the library's fill and compared with
    the model once), the model's copies on the host, the expected C and a
    ``launch(tile_xcd_ptr, counters_ptr)`` of the fused check.  Shared between the sweeps: every
    sweep leaves the operands as it found them."""
    gpu = _gpu()
    lib = gpu.load_library()
    m, n, k = SWEEP_SHAPE
    dev = torch.device("cuda", 0)
    code = ref.NAMES[fmt]
    p = types.SimpleNamespace(fmt=fmt, code=code, m=m, n=n, k=k, device=dev)
    a, bt, sa, sbt, table = _filled(dev, fmt, m, n, k)
    p.t = {"a": a, "bt": bt, "sa": sa, "sbt": sbt}
    p.values = ref.probe_values(m, n, k)
    p.host = {"a": ref.encode(code, p.values[0]), "bt": ref.encode(code, p.values[1]),
              "sa": ref.probe_scales(m, k), "sbt": ref.probe_scales(n, k)}
    p.expect = ref.probe_table(k)[np.arange(m)[:, None] % mx.ROWS, np.arange(n)[None, :] % mx.COLS]
    assert np.array_equal(table.cpu().double().numpy(), ref.probe_table(k))
    p.product = lambda h: ref.product(code, h["a"], h["bt"], h["sa"], h["sbt"])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch(tile_xcd, counters):
        gpu._check(lib.odh_mx_probe_gemm_verify(code, a.data_ptr(), bt.data_ptr(), sa.data_ptr(), sbt.data_ptr(),
                                                table.data_ptr(), m, n, k, tile_xcd, counters, stream))

    p.launch = launch
    _assert_operands_are_the_models(p)
    assert np.array_equal(p.product(p.host), p.expect)
    return p


def _assert_operands_are_the_models(p):
    for name, host in p.host.items():
        assert np.array_equal(p.t[name].cpu().numpy(), host), f"{p.fmt} {name} differs from the model"


def _sweep(p, name, wrong_host, rows):
    """``wrong_host`` is the model's ``name`` (``a``, ``bt``, ``sa`` or ``sbt``) with one element of
    every row changed (one or two adjacent bytes of a packed row).  Launch x runs with only row
    x's bytes changed, into counter row x and tile map x, and restores them; everything is read
    back once at the end.

    A changed element of row i of A (or of its scales) changes only row i of the product, so row
    i of the product of ``wrong_host`` with the other, clean operands is launch i's row i, and
    every other row of that launch is clean.  For Bt and its scales the same holds of columns."""
    gpu = _gpu()
    m, n = p.m, p.n
    tiles_m, tiles_n = m // 256, n // 256
    tiles = tiles_m * tiles_n
    count = m if rows else n
    target, clean_host = p.t[name], p.host[name]
    width = target.shape[1]
    assert (name in ("a", "sa")) == rows and wrong_host.shape == clean_host.shape == (count, width)
    diff = wrong_host != clean_host
    first = diff.argmax(axis=1)
    last = width - 1 - diff[:, ::-1].argmax(axis=1)
    assert diff.any(axis=1).all() and (last - first <= 1).all(), "one changed element per row"
    dev = p.device
    wrong_dev = torch.from_numpy(wrong_host).to(dev)
    clean_dev = torch.from_numpy(clean_host).to(dev)
    counters = torch.zeros((count, gpu.ODH_NCOUNT), dtype=torch.int32, device=dev)
    tile_xcd = torch.full((count, tiles), -1, dtype=torch.int32, device=dev)
    cp, tp = counters.data_ptr(), tile_xcd.data_ptr()
    try:
        for x in range(count):
            lo, hi = int(first[x]), int(last[x]) + 1
            target[x, lo:hi].copy_(wrong_dev[x, lo:hi])
            p.launch(tp + 4 * tiles * x, cp + 4 * gpu.ODH_NCOUNT * x)
            target[x, lo:hi].copy_(clean_dev[x, lo:hi])
    finally:
        target.copy_(clean_dev)  # the operands are shared between the sweeps
    h = counters.cpu().numpy()
    tx = tile_xcd.cpu().numpy()
    _assert_operands_are_the_models(p)

    mismatch = p.product(dict(p.host, **{name: wrong_host})) != p.expect  # [i][j]
    lines = mismatch if rows else mismatch.T  # [x][position along launch x's line]
    want_err = lines.sum(axis=1)
    assert (want_err > 0).all(), "a launch that expects no mismatch checks nothing"
    per_tile = lines.reshape(count, -1, 256).sum(axis=2)  # [x][tile along the line]
    assert ((tx >= 0) & (tx < gpu.N_XCD)).all(), tx[((tx < 0) | (tx >= gpu.N_XCD)).any(axis=1)][:4]
    want_xcd = np.zeros((count, gpu.N_XCD), dtype=np.int64)
    for x in range(count):
        for t in range(per_tile.shape[1]):
            tm, tn = (x // 256, t) if rows else (t, x // 256)
            want_xcd[x, tx[x, tm * tiles_n + tn]] += per_tile[x, t]
    what = f"{p.fmt} {name} " + ("row" if rows else "column")
    got_err = h[:, gpu.ODH_SLOT_GEMM_ERR].astype(np.int64) & 0xFFFFFFFF
    for x in np.flatnonzero(got_err != want_err)[:8]:
        print(f"{what} {x}: {got_err[x]} mismatches counted, {want_err[x]} expected")
    assert np.array_equal(got_err, want_err), f"{what}s {np.flatnonzero(got_err != want_err)[:16].tolist()}"
    got_xcd = h[:, gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.N_XCD]
    bad = np.flatnonzero((got_xcd != want_xcd).any(axis=1))
    assert bad.size == 0, f"{what} {bad[0]}: per-XCD {got_xcd[bad[0]].tolist()} != {want_xcd[bad[0]].tolist()}"
    blocks = h[:, gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + gpu.N_XCD]
    hist = np.stack([np.bincount(r, minlength=gpu.N_XCD) for r in tx])
    assert np.array_equal(blocks, hist) and (blocks.sum(axis=1) == tiles).all()
    return want_err


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_check_sees_every_row_and_column(dev, fmt, rows):
    """``A[i][i % 384]`` (``Bt[j][j % 384]``) is one value higher (-1 .. 3 and -2 .. 4 are exact in
    all three formats), one launch each, 512 launches: k runs through all four bit offsets of
    the packing and all three (BF8: six) stages, in every row and column of the 2 × 2 tiles.  A
    changed row is wrong in 438 or 439 of 512 columns and a changed column in 409 or 410 of 512
    rows, so a check that skips a register, a wave, a fragment or a tile, or books a tile on
    another XCD, miscounts some launch."""
    p = _probe(fmt)
    assert mx.zero_classes(p.k) == 0
    v = p.values[0 if rows else 1].copy()
    idx = np.arange(v.shape[0])
    hot = idx % p.k
    assert set((hot % 4).tolist()) == {0, 1, 2, 3} and set((hot // 128).tolist()) == {0, 1, 2}
    v[idx, hot] += 1
    name = "a" if rows else "bt"
    wrong = ref.encode(p.code, v)
    if fmt in PACKED:  # only the one element changed
        was, now = ref.unpack6(p.host[name]), ref.unpack6(wrong)
        assert np.array_equal(np.argwhere(was != now), np.stack([idx, hot], axis=1))
    want = _sweep(p, name, wrong, rows)
    assert set(want.tolist()) <= ({438, 439} if rows else {409, 410})


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", PACKED)
def test_fused_check_reads_every_scale_byte(dev, fmt, rows):
    """``sA[i][i % 12]`` (``sBt[j][j % 12]``) goes up by one, which doubles that block.  The 12
    blocks of a row are the four scale bytes of each of the three stages: both lane halves and
    both ``opsel`` bytes, in every row of the tile."""
    p = _probe(fmt)
    name = "sa" if rows else "sbt"
    wrong = p.host[name].copy()
    idx = np.arange(wrong.shape[0])
    assert wrong.shape[1] == 12
    wrong[idx, idx % 12] += 1
    want = _sweep(p, name, wrong, rows)
    assert want.min() >= (438 if rows else 409) and want.max() <= 512  # of the model: no launch is vacuous


# ------------------------------------------------------------------ the program


def _run_probe(*args, timeout=120):
    from odh_kubeflow_amd.ops import probe_main

    exe = probe_main.executable()
    if not os.path.exists(exe):
        pytest.fail("odh-gpu-probe not built: python -m odh_kubeflow_amd.ops.build")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("HIP_VISIBLE", "ROCR_VISIBLE", "CUDA_VISIBLE"))}
    env["HIP_VISIBLE_DEVICES"] = "0"
    r = subprocess.run(["timeout", "-k", "10", str(timeout), exe, "--json", "-", *args], capture_output=True,
                       text=True, env=env, timeout=timeout + 20)
    return r.returncode, probe_main.parse_result(r.stdout), r


def test_program_checks_all_five_formats():
    """Everything on at once on one GPU: the verdict still fits the kubelet's 4096-byte termination
    message."""
    rc, res, r = _run_probe("--mx", ",".join(ALL_FIVE), "--dtypes", "f16,i8", "--rccl-mib", "16")
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["mx"]) == ALL_FIVE  # one entry per format, in the order given
    for fmt in ALL_FIVE:
        f = res["mx"][fmt]
        assert f["ok"] is True and f["errors"] == 0, res["mx"]
        assert f["tflops"] > 50 and f["ms"] > 0 and f["host_ms"] > 0, res["mx"]  # the matrix cores, not a stub
    assert set(res["dtypes"]) == {"f16", "i8"} and res["rccl"]["ok"] is True
    d = res["results"][0]
    assert d["gemm_errors"] == 0 and d["hbm_errors"] == 0
    line = r.stdout.strip().splitlines()[-1]
    assert len(line.encode()) < 4096, len(line.encode())
    print("verdict bytes:", len(line.encode()), "mx:", json.dumps(res["mx"]), "timings_ms:", json.dumps(res["timings_ms"]))


def test_program_fails_every_format_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--mx", ",".join(ALL_FIVE), "--shape", "256,256,256", "--inject-fault", "mx")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    want = sum(1 for j in range(256) if (11 * j) % 7 != 3)
    assert want == 220
    assert res["ok"] is False and list(res["mx"]) == ALL_FIVE
    for fmt in ALL_FIVE:
        assert res["mx"][fmt]["ok"] is False and res["mx"][fmt]["errors"] == want, res["mx"]
    assert "GPU 0" in res["error"] and "fp8" in res["error"] and "XCD" in res["error"], res["error"]
    d = res["results"][0]
    assert d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1].encode()) < 4096
