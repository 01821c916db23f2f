"""What the GPU test files of the probe's matrix-core kernels share (``test_gpu_mx_exact.py``,
``test_gpu_mx_formats_exact.py``, ``test_gpu_dense_exact.py``, ``test_gpu_lowprec_sweeps.py``,
``test_gpu_sparse_fp_sweeps.py``): the device fixture and the per-test timeout, which they import by name, the probe operands of a
format next to their host model, the sweeps that change one element per launch, the store
checks, and the run of ``odh-gpu-probe``.

The tests corrupt data only; every pointer handed to a kernel comes from a torch allocation of
exactly the size the shape implies (a launch's counter row and tile map are rows of such an
allocation).
"""

import faulthandler
import functools
import os
import subprocess
import types

import numpy as np
import pytest

import fp_reference as fp
import mx_reference as mx
import probe_reference as ref
import sparse_reference as sp

torch = pytest.importorskip("torch")

TEST_TIMEOUT_S = 60  # per test: a hung kernel ends the run here instead of holding the GPU
NP_DTYPE = {"f16": np.float16, "i8": np.int8}
I8_MUL = {"a": 25, "bt": 41}


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


# ------------------------------------------------------------------ the probe operands and their model


def _mx_filled(dev, fmt, m, n, k):
    """Operands, scales and table of the MX probe, written by the library's fill over a pattern."""
    gpu = _gpu()
    rb = gpu.mx_row_bytes(fmt, k)
    a = torch.full((m, rb), 0xEE, dtype=torch.uint8, device=dev)
    bt = torch.full((n, rb), 0xEE, dtype=torch.uint8, device=dev)
    sa = torch.zeros((m, k // 32), dtype=torch.uint8, device=dev)
    sbt = torch.zeros((n, k // 32), dtype=torch.uint8, device=dev)
    table = torch.full(gpu.MX_TABLE, float("nan"), device=dev)
    gpu.mx_fill(fmt, a, bt, sa, sbt, table)
    return a, bt, sa, sbt, table


@functools.lru_cache(maxsize=None)
def _probe(fmt, m, n, k):
    """The probe operands of ``fmt`` on the GPU (written by the library's fill and compared with
    the model once), the model's copies on the host, the expected C, a ``product(host)`` that
    multiplies host operands in float64 / int64, and a ``launch(tile_xcd_ptr, counters_ptr)`` of
    the fused check.  Shared between tests: every test leaves the operands as it found them.

    ``fmt`` names an MX format, ``f16`` / ``i8`` (dense), ``f32`` / ``f64``, or a 2:4 sparse format as
    ``sp:bf16``, ``sp:f16``, ``sp:i8``, ``sp:fp8``, ``sp:bf8``.  The sparse tensors ``ac``, ``meta``, ``bt`` and their
    host copies are the elements as stored (``sparse_reference.NP_STORED``: bf16 as the int16 of its bits,
    fp8 and bf8 as codes), so that numpy holds them.  ``tile_n`` is the width of a workgroup's tile."""
    gpu = _gpu()
    lib = gpu.load_library()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = types.SimpleNamespace(fmt=fmt, m=m, n=n, k=k, device=dev, tile_n=256)
    if fmt.startswith("sp:"):
        sfmt = fmt[3:]
        code = gpu.SPARSE_FORMATS[sfmt]
        dtype = gpu._sparse_dtype(code)
        ac = torch.zeros((m, k // 2), dtype=dtype, device=dev)
        meta = torch.full((m, k // 8), 0x77, dtype=torch.uint8, device=dev)
        bt = torch.zeros((n, k), dtype=dtype, device=dev)
        table = torch.full(gpu.SPARSE_TABLE, -1, dtype=torch.int32, device=dev)
        gpu.sparse_fill(sfmt, ac, meta, bt, table)
        stored = torch.from_numpy(np.zeros(1, dtype=sp.NP_STORED[sfmt])).dtype
        t = {"ac": ac.view(stored), "meta": meta, "bt": bt.view(stored)}
        hac, hmeta, hbt = sp.fill(sfmt, m, n, k)
        p.values = (hac, hbt)
        p.host = {"ac": sp.encode(sfmt, hac), "meta": hmeta, "bt": sp.encode(sfmt, hbt)}
        p.expect = sp.expected(sfmt, m, n, k)
        assert np.array_equal(table.cpu().numpy().astype(np.int64), sp.table(k))
        # times nothing: the fill has applied the i8 multipliers
        p.product = lambda h: sp.product(sp.decode(sfmt, h["ac"]), h["meta"], sp.decode(sfmt, h["bt"]))

        def launch(tile_xcd, counters):
            gpu._check(lib.odh_sparse_probe_gemm_verify(code, ac.data_ptr(), meta.data_ptr(), bt.data_ptr(),
                                                        table.data_ptr(), m, n, k, tile_xcd, counters, stream))
    elif fmt in fp.FORMATS:
        code = gpu.FP_FORMATS[fmt]
        p.tile_n = fp.TILE_N[fmt]
        dtype = torch.float64 if fmt == "f64" else torch.float32
        t = {"a": torch.full((m, k), 77, dtype=dtype, device=dev), "bt": torch.full((n, k), 77, dtype=dtype, device=dev)}
        gpu.fp_fill(fmt, t["a"], t["bt"])
        p.values = fp.operand_values(fmt, m, n, k)
        p.host = dict(zip(("a", "bt"), fp.operands(fmt, m, n, k)))
        p.expect = fp.expected(fmt, m, n, k)
        p.product = lambda h: h["a"].astype(np.int64) @ h["bt"].astype(np.int64).T

        def launch(tile_xcd, counters):
            gpu._check(lib.odh_fp_probe_gemm_verify(code, t["a"].data_ptr(), t["bt"].data_ptr(), m, n, k,
                                                    tile_xcd, counters, stream))
    elif fmt in mx.NAMES:
        code = p.code = mx.NAMES[fmt]
        a, bt, sa, sbt, table = _mx_filled(dev, fmt, m, n, k)
        t = {"a": a, "bt": bt, "sa": sa, "sbt": sbt}
        p.values = mx.probe_values(m, n, k)
        p.host = {"a": mx.encode(code, p.values[0]), "bt": mx.encode(code, p.values[1]),
                  "sa": mx.probe_scales(m, k), "sbt": mx.probe_scales(n, k)}
        p.expect = mx.probe_table(k)[np.arange(m)[:, None] % mx.ROWS, np.arange(n)[None, :] % mx.COLS]
        assert np.array_equal(table.cpu().double().numpy(), mx.probe_table(k))
        p.product = lambda h: mx.product(code, h["a"], h["bt"], h["sa"], h["sbt"])

        def launch(tile_xcd, counters):
            gpu._check(lib.odh_mx_probe_gemm_verify(code, a.data_ptr(), bt.data_ptr(), sa.data_ptr(), sbt.data_ptr(),
                                                    table.data_ptr(), m, n, k, tile_xcd, counters, stream))
    else:
        code = gpu.DENSE_FORMATS[fmt]
        dtype = torch.int8 if fmt == "i8" else torch.float16
        t = {"a": torch.full((m, k), 77, dtype=dtype, device=dev), "bt": torch.full((n, k), 77, dtype=dtype, device=dev)}
        gpu.dense_fill(fmt, t["a"], t["bt"])
        va, vb = ref.probe_operands(m, n, k)
        mul = (gpu.ODH_DT_I8_MUL_A, gpu.ODH_DT_I8_MUL_B) if fmt == "i8" else (1, 1)
        assert fmt != "i8" or mul == (I8_MUL["a"], I8_MUL["bt"])
        p.values = (va * mul[0], vb * mul[1])
        p.host = {"a": p.values[0].astype(NP_DTYPE[fmt]), "bt": p.values[1].astype(NP_DTYPE[fmt])}
        p.expect = (ref.probe_class_table(k) * mul[0] * mul[1])[np.arange(m)[:, None] % 5, np.arange(n)[None, :] % 7]
        wide = np.int64 if fmt == "i8" else np.float64  # float64 holds the halves' inf and NaN too
        p.product = lambda h: h["a"].astype(wide) @ h["bt"].astype(wide).T

        def launch(tile_xcd, counters):
            gpu._check(lib.odh_dense_probe_gemm_verify(code, t["a"].data_ptr(), t["bt"].data_ptr(), m, n, k,
                                                       tile_xcd, counters, stream))
    p.t, p.launch = t, launch
    _assert_operands_are_the_models(p)
    # the model agrees with itself: the clean product is the table, so a launch's mismatches are
    # exactly those of the one line its corrupted element touches
    assert np.array_equal(p.product(p.host), p.expect)
    return p


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _assert_operands_are_the_models(p):
    for name, host in p.host.items():
        assert np.array_equal(_bits(p.t[name].cpu().numpy()), _bits(host)), f"{p.fmt} {name} differs from the model"


ROW_OPERANDS = {"a", "sa", "ac", "meta"}  # a changed element of row i changes row i of the product
COLUMN_OPERANDS = {"bt", "sbt"}


def _sweep(p, name, wrong_host, rows):
    """``wrong_host`` is the model's ``name`` (``a``, ``bt``, ``sa``, ``sbt``, or the sparse ``ac`` or ``meta``) with
    one element of every row changed: one array element, one or two adjacent bytes of a packed
    6-bit row, or the metadata byte that holds a changed nibble.
    Launch x runs with only row x's element changed, into counter row x and tile map x, and
    restores it; everything is read back once at the end.

    A changed element of row i of A (or of its scales) changes only row i of the product, so row
    i of the product of ``wrong_host`` with the other, clean operands is launch i's row i, and
    every other row of that launch is clean.  For Bt and its scales the same holds of columns.

    A workgroup's tile is 256 rows by ``p.tile_n`` columns (128 for f64), so a row's line crosses tiles
    of ``p.tile_n`` and a column's line tiles of 256; every kernel books tile ``(tm, tn)`` at
    ``tile_xcd[tm * tiles_n + tn]``."""
    gpu = _gpu()
    m, n = p.m, p.n
    tile_n = p.tile_n
    tiles_m, tiles_n = m // 256, n // tile_n
    tiles = tiles_m * tiles_n
    count = m if rows else n
    target, clean_host = p.t[name], p.host[name]
    width = target.shape[1]
    assert name in ROW_OPERANDS | COLUMN_OPERANDS and (name in ROW_OPERANDS) == rows
    assert wrong_host.shape == clean_host.shape == (count, width) and wrong_host.dtype == clean_host.dtype
    diff = wrong_host != clean_host
    first = diff.argmax(axis=1)
    last = width - 1 - diff[:, ::-1].argmax(axis=1)
    widest = 2 if name in ("a", "bt") and getattr(p, "code", None) in mx.PACKED else 1
    assert diff.any(axis=1).all() and (last - first < widest).all(), "one changed element per row"
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
        target.copy_(clean_dev)  # the operands are shared between tests
    h = counters.cpu().numpy()
    tx = tile_xcd.cpu().numpy()
    _assert_operands_are_the_models(p)

    mismatch = p.product(dict(p.host, **{name: wrong_host})) != p.expect  # [i][j]
    lines = mismatch if rows else mismatch.T  # [x][position along launch x's line]
    want_err = lines.sum(axis=1)
    assert (want_err > 0).all(), "a launch that expects no mismatch checks nothing"
    per_tile = lines.reshape(count, -1, tile_n if rows else 256).sum(axis=2)  # [x][tile along the line]
    assert per_tile.shape[1] == (tiles_n if rows else tiles_m)
    assert ((tx >= 0) & (tx < gpu.N_XCD)).all(), tx[((tx < 0) | (tx >= gpu.N_XCD)).any(axis=1)][:4]
    want_xcd = np.zeros((count, gpu.N_XCD), dtype=np.int64)
    for x in range(count):
        for t in range(per_tile.shape[1]):
            tm, tn = (x // 256, t) if rows else (t, x // tile_n)
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


# ------------------------------------------------------------------ the sweeps, for any format

MX_FORMATS = ["fp8", "fp4", "bf8", "fp6", "bf6"]
# 2 × 2 tiles, so tm and tn are both non-zero somewhere.  fp8 / bf8: 6 stages, fp4 / fp6 / bf6: 3, odd
# and even stages on both buffers, no class expecting 0; f16 / i8: 5 stages, so the ring is refilled
SWEEP_SHAPE = dict({fmt: (512, 512, 384) for fmt in MX_FORMATS}, f16=(512, 512, 160), i8=(512, 512, 320))


def _wrap_i8(x):
    return ((np.asarray(x, dtype=np.int64) + 128) % 256 - 128).astype(np.int8)


def _value_plus_one(p, rows):
    """The model's A (or Bt) with ``A[i][i % K]`` (``Bt[j][j % K]``) one value higher, re-encoded:
    -1 .. 3 and -2 .. 4 stay exact in all seven formats (FP4 has 3 and 4).  For i8 one higher means
    plus the multiplier, 25 or 41; ``Bt = 3 · 41 + 41 = 164`` does not fit and wraps to -92, and
    the model multiplies the int8 that is stored.  The FP4 neighbour nibble and the packed 6-bit
    neighbours are re-encoded unchanged with it."""
    v = p.values[0 if rows else 1].copy()
    idx = np.arange(v.shape[0])
    name = "a" if rows else "bt"
    if p.fmt in MX_FORMATS:
        hot = idx % p.k
        # k runs through all four bit offsets of the 6-bit packing and all three 128-element stages
        assert set((hot % 4).tolist()) == {0, 1, 2, 3} and set((hot // 128).tolist()) == {0, 1, 2}
        v[idx, hot] += 1
        wrong = mx.encode(p.code, v)
        if p.code in mx.PACKED:  # only the one element changed
            was, now = mx.unpack6(p.host[name]), mx.unpack6(wrong)
            assert np.array_equal(np.argwhere(was != now), np.stack([idx, hot], axis=1))
        if p.fmt == "fp4":  # only the one nibble changed
            x = (wrong ^ p.host[name])[idx, (idx % p.k) // 2]
            shift = 4 * ((idx % p.k) & 1)
            assert ((x >> shift) & 15).all() and not ((x >> (4 - shift)) & 15).any()
        return name, wrong
    if p.fmt == "i8":
        v[idx, idx % p.k] += I8_MUL[name]
        return name, _wrap_i8(v)
    v[idx, idx % p.k] += 1
    return name, v.astype(np.float16)


def sweep_every_row_and_column(fmt, rows):
    """One operand element per launch, 512 launches.  With the probe operands a changed row is
    wrong in 438 or 439 of 512 columns and a changed column in 409 or 410 of 512 rows (the zeros
    of the other operand at that k are not), so a check that skips a register, a wave, a
    fragment or a tile, or books a tile on another XCD, miscounts some launch."""
    p = _probe(fmt, *SWEEP_SHAPE[fmt])
    if fmt in MX_FORMATS:
        assert mx.zero_classes(p.k) == 0
    else:
        assert p.k % ref.PERIOD != 0
    want = _sweep(p, *_value_plus_one(p, rows), rows)
    assert set(want.tolist()) <= ({438, 439} if rows else {409, 410})


def sweep_every_scale_byte(fmt, rows):
    """``sA[i][i % (K/32)]`` (``sBt[j][j % (K/32)]``) goes up by one, which doubles that block.  The
    12 blocks of a row are every scale byte of a stage (2 for FP8 and BF8, 4 for FP4, FP6 and BF6),
    both lane halves and both ``opsel`` bytes, in every row of the tile."""
    p = _probe(fmt, *SWEEP_SHAPE[fmt])
    name = "sa" if rows else "sbt"
    wrong = p.host[name].copy()
    idx = np.arange(wrong.shape[0])
    assert wrong.shape[1] == 12
    wrong[idx, idx % 12] += 1
    want = _sweep(p, name, wrong, rows)
    assert want.min() >= (438 if rows else 409) and want.max() <= 512  # of the model: no launch is vacuous


# ------------------------------------------------------------------ store kernels


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


def store_decodes_every_code(dev, fmt):
    """All 256 × 256 pairs of FP8 codes (subnormals, fractional mantissas, ±448 and the two NaN
    codes included) and of BF8 codes (subnormals, ±57344, both infinities and the six NaN codes
    included; the MI355X agrees with the model's IEEE product on the infinities too, inf · x =
    ±inf and inf · 0 = NaN, so no exception is listed); all 16 × 16 pairs of FP4 codes sixteen
    times over; all 64 × 64 pairs of FP6 / BF6 codes sixteen times over, at all 128 positions of a
    stage.  Seeded scales 2^-8 .. 2^8: each output is one product,
    ``decode(i) · decode(j) · 2^(sA + sBt - 254)``."""
    got, want = _mx_store(dev, fmt, mx.all_codes_case(mx.NAMES[fmt]))
    _assert_store_exact(f"{fmt} code i × code j", got, want)


def store_applies_every_scale_byte(dev, fmt):
    """E8M0 bytes 1 .. 254 through the scale loads of the 8-bit arms (FP8) or of the 6-bit arms
    (FP6: one u32 per row and stage, 64 stages): 1.0 · 1.0 under ``sA = i`` and an ``sBt`` that brings
    the pair back to 2^-20 .. 2^20; every output is that power of two."""
    got, want = _mx_store(dev, fmt, mx.e8m0_range_case(mx.NAMES[fmt]))
    _assert_store_exact(f"{fmt} scale i", got, want)


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
