"""The probe library's kernels on a real MI355X against the host model (``probe_reference.py``).

Nearly everything here is bit-exact: small-integer bf16 operands make every GEMM result
exact in fp32 whatever the summation order, and the HBM pattern is integer arithmetic.  The
tests corrupt data only; every pointer handed to a kernel is 16-byte aligned and covers the
length passed with it.
"""

import functools

import numpy as np
import pytest

import probe_reference as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD_WORDS = 64  # int32 words on each side of an HBM test buffer
GUARD = 0xA5A5A5A5 - (1 << 32)  # as int32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from odh_kubeflow_amd.ops import gpu

    gpu.load_library()  # loud failure if the in-tree .so is missing
    return torch.device("cuda", 0)


def _lib():
    from odh_kubeflow_amd.ops import gpu

    return gpu, gpu.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ 3a. GEMM store kernels


@functools.lru_cache(maxsize=None)
def _int_case(m, n, k):
    """Seeded integer operands in [-8, 8] (exact in bf16) and their float64 product on the CPU:
    ``|sum| <= 64 K < 2^24``, so fp32 accumulation is exact in any order."""
    g = torch.Generator().manual_seed(1000003 * m + 1009 * n + k)
    a = torch.randint(-8, 9, (m, k), generator=g, dtype=torch.int32)
    bt = torch.randint(-8, 9, (n, k), generator=g, dtype=torch.int32)
    return a.to(torch.bfloat16), bt.to(torch.bfloat16), a.double() @ bt.double().t()


def _launch_store(kernel, a, bt, c, tile_xcd=None, xcd_blocks=None):
    gpu, lib = _lib()
    m, k = a.shape
    n = bt.shape[0]
    tx = tile_xcd.data_ptr() if tile_xcd is not None else None
    xb = xcd_blocks.data_ptr() if xcd_blocks is not None else None
    if kernel == "auto":
        rc = lib.odh_gemm_bf16(a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, tx, xb, _stream())
    elif kernel == "128":
        rc = lib.odh_gemm_bf16_128(a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, tx, xb, _stream())
    else:
        rc = lib.odh_gemm_bf16_256_variant(a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, int(kernel[1:]),
                                           _stream())
    gpu._check(rc)


def _exact_store(dev, kernel, m, n, k):
    a, bt, want = _int_case(m, n, k)
    c = torch.full((m, n), float("nan"), device=dev)
    _launch_store(kernel, a.to(dev), bt.to(dev), c)
    got = c.cpu().double()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        pytest.fail(f"{kernel} {m}x{n}x{k}: {len(bad)} wrong elements, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}")


# 1, 2, 3 and 5 K-tiles; 15 tiles (no remap, non-square); 8 tiles (remap); 16 tiles (remap, tiles_n = 2)
SHAPES_128 = [(128, 128, 32), (128, 128, 64), (128, 128, 96), (128, 128, 160),
              (384, 640, 32), (256, 512, 32), (1024, 256, 32)]
# K-tiles 1..5 of the 2-buffer kernel = stages 2, 4 (ring depth), 6, 8, 10 of the deep ring (in its
# cross-barrier form: no refill, kt+4 only, both refills) and a long K; then grids at K=64 with
# nwg % 8 = 0, 1, 7 (nwg > 8) and a single tile row of 11
SHAPES_256 = [(256, 256, 64), (256, 256, 128), (256, 256, 192), (256, 256, 256), (256, 256, 320), (256, 256, 4096),
              (512, 1024, 64), (768, 768, 64), (1280, 768, 64), (256, 2816, 64)]


@pytest.mark.parametrize("m,n,k", SHAPES_128)
def test_gemm128_exact(dev, m, n, k):
    _exact_store(dev, "128", m, n, k)


@pytest.mark.parametrize("kernel", ["auto", "v0", "v1", "v2", "v3"])
@pytest.mark.parametrize("m,n,k", SHAPES_256)
def test_gemm256_exact(dev, kernel, m, n, k):
    _exact_store(dev, kernel, m, n, k)


@pytest.mark.parametrize("m,n,k", [s for s in SHAPES_128 if s[0] % 256 or s[1] % 256 or s[2] % 64])
def test_gemm_auto_exact_on_128_shapes(dev, m, n, k):
    """``odh_gemm_bf16`` takes the 128² kernel where the 256² tile does not divide the shape."""
    _exact_store(dev, "auto", m, n, k)


@pytest.mark.parametrize("kernel,m,n,k", [(kern, *s) for kern in ("128", "auto") for s in SHAPES_128[4:]] +
                         [("auto", *s) for s in SHAPES_256[6:]])
def test_gemm_tile_xcd_map(dev, kernel, m, n, k):
    """Every tile records the XCD it ran on exactly once: the first ``tiles`` entries are 0..7,
    the rest untouched, and their histogram is ``xcd_blocks``."""
    gpu, lib = _lib()
    a, bt, want = _int_case(m, n, k)
    tiles = (m // 128) * (n // 128) if kernel == "128" else lib.odh_gemm_tiles(m, n, k)
    assert tiles == ((m // 256) * (n // 256) if kernel == "auto" and gpu.fused_verify_ok(m, n, k)
                     else (m // 128) * (n // 128))
    tile_xcd = torch.full(((m // 128) * (n // 128) + 8,), -1, dtype=torch.int32, device=dev)
    xcd_blocks = torch.zeros((gpu.N_XCD,), dtype=torch.int32, device=dev)
    c = torch.full((m, n), float("nan"), device=dev)
    _launch_store(kernel, a.to(dev), bt.to(dev), c, tile_xcd, xcd_blocks)
    assert torch.equal(c.cpu().double(), want)
    tx = tile_xcd.cpu().numpy()
    assert ((tx[:tiles] >= 0) & (tx[:tiles] < gpu.N_XCD)).all(), tx
    assert (tx[tiles:] == -1).all(), tx
    assert np.bincount(tx[:tiles], minlength=gpu.N_XCD).tolist() == xcd_blocks.cpu().tolist()


@pytest.mark.parametrize("kernel", ["auto", "128", "v0", "v1", "v2", "v3"])
def test_gemm_randn_within_accumulation_bound(dev, kernel):
    """bf16 × bf16 products are exact in fp32, so the error is accumulation only: elementwise
    ``|c - ref| <= K 2^-23 (|A| |Bt|ᵀ)``, the standard ``K u`` bound with the unit roundoff
    doubled (2^-23) to allow an accumulator that truncates; the float64 reference's own error,
    ``K 2^-53`` relative, is nine orders below it."""
    m, n, k = 256, 512, 1024
    g = torch.Generator().manual_seed(20240 + k)
    a = torch.randn((m, k), generator=g).to(torch.bfloat16)
    bt = torch.randn((n, k), generator=g).to(torch.bfloat16)
    want = a.double() @ bt.double().t()
    bound = k * 2.0 ** -23 * (a.double().abs() @ bt.double().abs().t())
    c = torch.full((m, n), float("nan"), device=dev)
    _launch_store(kernel, a.to(dev), bt.to(dev), c)
    got = c.cpu().double()
    assert not torch.isnan(got).any()
    ratio = ((got - want).abs() / bound).max().item()
    print(f"{kernel}: max |c - ref| / bound = {ratio:.3e}, max |c - ref| = {(got - want).abs().max().item():.3e}")
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------ 3b. operands, store + check


def test_probe_fill_store_and_check_kernel(dev):
    gpu, lib = _lib()
    m, n, k = 384, 640, 96
    a = torch.full((m, k), float("nan"), dtype=torch.bfloat16, device=dev)
    bt = torch.full((n, k), float("nan"), dtype=torch.bfloat16, device=dev)
    gpu._check(lib.odh_probe_fill(a.data_ptr(), bt.data_ptr(), m, n, k, _stream()))
    ha, hbt = ref.probe_operands(m, n, k)
    assert np.array_equal(a.cpu().double().numpy(), ha.astype(np.float64))
    assert np.array_equal(bt.cpu().double().numpy(), hbt.astype(np.float64))

    c = torch.full((m, n), float("nan"), device=dev)
    _launch_store("128", a, bt, c)
    want = ref.probe_expected(m, n, k)
    assert np.array_equal(c.cpu().double().numpy(), want.astype(np.float64))

    tiles_m, tiles_n = m // 128, n // 128
    tile_xcd = torch.tensor([(5 * t + 3) % 8 for t in range(tiles_m * tiles_n)], dtype=torch.int32, device=dev)
    counters = torch.zeros((2, gpu.ODH_NCOUNT), dtype=torch.int32, device=dev)

    def verify(row):
        p = counters[row].data_ptr()
        gpu._check(lib.odh_probe_verify(c.data_ptr(), m, n, k, tile_xcd.data_ptr(), p + 4 * gpu.ODH_SLOT_GEMM_ERR,
                                        p + 4 * gpu.ODH_SLOT_ERR_XCD, _stream()))

    verify(0)
    # one wrong element in every 128² tile (a different place in each), the last element, a NaN, an inf
    planted = [(tm * 128 + (37 * (tm * tiles_n + tn) + 5) % 128, tn * 128 + (53 * (tm * tiles_n + tn) + 11) % 128, None)
               for tm in range(tiles_m) for tn in range(tiles_n)]
    planted += [(m - 1, n - 1, None), (200, 300, float("nan")), (130, 639, float("inf"))]
    assert len({(i, j) for i, j, _ in planted}) == len(planted)
    want_xcd = [0] * gpu.N_XCD
    for i, j, v in planted:
        c[i, j] = float(want[i, j] + 1) if v is None else v
        want_xcd[(5 * ((i // 128) * tiles_n + j // 128) + 3) % 8] += 1
    verify(1)
    h = counters.cpu().tolist()
    assert h[0] == [0] * gpu.ODH_NCOUNT
    assert h[1][gpu.ODH_SLOT_GEMM_ERR] == len(planted)
    assert h[1][gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.N_XCD] == want_xcd


# ------------------------------------------------------------------ 3c. fused verify

ENTRY_POINTS = ["probe", "2buf"] + [f"deep{v}" for v in range(8)]


def _gm_of(entry):
    return 1 << (int(entry[4:]) >> 1) if entry.startswith("deep") else 1


def _fused_launch(entry, a, bt, m, n, k, tile_xcd, counters_row_ptr):
    gpu, lib = _lib()
    args = (a.data_ptr(), bt.data_ptr(), m, n, k, tile_xcd, counters_row_ptr + 4 * gpu.ODH_SLOT_XCD_BLOCKS,
            counters_row_ptr + 4 * gpu.ODH_SLOT_GEMM_ERR, counters_row_ptr + 4 * gpu.ODH_SLOT_ERR_XCD)
    if entry == "probe":
        rc = lib.odh_probe_gemm_verify(*args, _stream())
    elif entry == "2buf":
        rc = lib.odh_probe_gemm_verify_2buf(*args, _stream())
    else:
        rc = lib.odh_probe_gemm_verify_deep(*args, int(entry[4:]), _stream())
    gpu._check(rc)


@functools.lru_cache(maxsize=None)
def _filled(m, n, k):
    """Probe operands on the GPU, checked once against the host model."""
    gpu, lib = _lib()
    a = torch.empty((m, k), dtype=torch.bfloat16, device="cuda:0")
    bt = torch.empty((n, k), dtype=torch.bfloat16, device="cuda:0")
    gpu._check(lib.odh_probe_fill(a.data_ptr(), bt.data_ptr(), m, n, k, _stream()))
    ha, hbt = ref.probe_operands(m, n, k)
    assert np.array_equal(a.cpu().double().numpy(), ha.astype(np.float64))
    assert np.array_equal(bt.cpu().double().numpy(), hbt.astype(np.float64))
    return a, bt, ha, hbt


FUSED_SHAPES = [(512, 512, 128), (1024, 256, 64), (2048, 512, 64), (256, 256, 2240)]


@pytest.mark.parametrize("entry", ENTRY_POINTS)
@pytest.mark.parametrize("m,n,k", FUSED_SHAPES)
def test_fused_verify_clean(dev, entry, m, n, k):
    """No mismatch on correct operands, every tile run exactly once.  At K = 2240 the
    expectation is all zero (``rem == 0`` of the closed form)."""
    gpu, _ = _lib()
    a, bt, _, _ = _filled(m, n, k)
    tiles = (m // 256) * (n // 256)
    tile_xcd = torch.full((tiles + 8,), -1, dtype=torch.int32, device=dev)
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    _fused_launch(entry, a, bt, m, n, k, tile_xcd.data_ptr(), counters.data_ptr())
    h = counters.cpu().tolist()
    tx = tile_xcd.cpu().numpy()
    assert h[gpu.ODH_SLOT_GEMM_ERR] == 0 and h[gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.N_XCD] == [0] * 8
    assert ((tx[:tiles] >= 0) & (tx[:tiles] < 8)).all() and (tx[tiles:] == -1).all(), tx
    assert h[gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + 8] == np.bincount(tx[:tiles], minlength=8).tolist()
    assert sum(h[gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + 8]) == tiles


def _sweep(dev, entry, m, n, k, rows):
    """Corrupt one operand element per launch — ``A[i][i % K]`` for every row i (``rows``) or
    ``Bt[j][j % K]`` for every column j — each launch into a counter row and a tile map of its
    own, restore, and read everything back once.  Adding 1 keeps the value exact (A: -1..3,
    Bt: -2..4).  Row i is then wrong exactly where ``Bt[j][i % K] != 0``; the mismatches of
    each 256-column tile belong to the XCD that ran that tile in that launch."""
    gpu, _ = _lib()
    a, bt, ha, hbt = _filled(m, n, k)
    tiles_m, tiles_n = m // 256, n // 256
    tiles = tiles_m * tiles_n
    count = m if rows else n
    target, host = (a, ha) if rows else (bt, hbt)
    idx = np.arange(count)
    flat = torch.from_numpy(idx * k + idx % k).to(dev)
    clean = torch.from_numpy(host[idx, idx % k].astype(np.float32)).to(dev).to(torch.bfloat16)
    wrong = torch.from_numpy((host[idx, idx % k] + 1).astype(np.float32)).to(dev).to(torch.bfloat16)
    tflat = target.view(-1)
    counters = torch.zeros((count, gpu.ODH_NCOUNT), dtype=torch.int32, device=dev)
    tile_xcd = torch.full((count, tiles), -1, dtype=torch.int32, device=dev)
    cp, tp = counters.data_ptr(), tile_xcd.data_ptr()
    offs = flat.cpu().tolist()
    try:
        for x in range(count):
            tflat[offs[x]:offs[x] + 1].copy_(wrong[x:x + 1])
            _fused_launch(entry, a, bt, m, n, k, tp + 4 * tiles * x, cp + 4 * gpu.ODH_NCOUNT * x)
            tflat[offs[x]:offs[x] + 1].copy_(clean[x:x + 1])
    finally:
        tflat[flat] = clean  # the operands are shared between tests
    h = counters.cpu().numpy()
    tx = tile_xcd.cpu().numpy()
    assert np.array_equal(target.cpu().double().numpy(), host.astype(np.float64))

    other = (hbt if rows else ha)[:, idx % k] != 0  # [j or i][x]: where launch x's line is wrong
    gm = _gm_of(entry)
    want_err = other.sum(axis=0)
    want_xcd = np.zeros((count, gpu.N_XCD), dtype=np.int64)
    per_tile = other.reshape(-1, 256, count).sum(axis=1)  # [tile along the line][x]
    for x in range(count):
        for t in range(per_tile.shape[0]):
            tm, tn = (x // 256, t) if rows else (t, x // 256)
            xcd = tx[x, ref.fused_tile_id(tm, tn, tiles_m, tiles_n, gm)]
            assert 0 <= xcd < gpu.N_XCD, (x, tx[x])
            want_xcd[x, xcd] += per_tile[t, x]
    what = "row" if rows else "column"
    got_err = h[:, gpu.ODH_SLOT_GEMM_ERR]
    for x in np.flatnonzero(got_err != want_err)[:8]:
        print(f"{entry} {m}x{n}x{k}: {what} {x}: {got_err[x]} mismatches counted, {want_err[x]} expected")
    assert np.array_equal(got_err, want_err), f"{what}s {np.flatnonzero(got_err != want_err)[:16].tolist()}"
    got_xcd = h[:, gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.N_XCD]
    bad = np.flatnonzero((got_xcd != want_xcd).any(axis=1))
    assert bad.size == 0, f"{what} {bad[0]}: per-XCD {got_xcd[bad[0]].tolist()} != {want_xcd[bad[0]].tolist()}"
    blocks = h[:, gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + gpu.N_XCD]
    assert (blocks.sum(axis=1) == tiles).all()


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_fused_verify_sees_every_row_and_column_512x512(dev, entry, rows):
    """2 × 2 tiles, 4 deep stages; ``GM = 2`` groups, ``GM = 4`` and ``8`` fall back to row-major."""
    _sweep(dev, entry, 512, 512, 128, rows)


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("entry,m,n,k", [("deep4", 1024, 256, 64), ("deep5", 1024, 256, 64),
                                         ("deep6", 2048, 512, 64), ("deep7", 2048, 512, 64)])
def test_fused_verify_sees_every_row_and_column_grouped_tiles(dev, entry, m, n, k, rows):
    """Shapes at which tile grouping ``GM = 4`` (one column of 4 tiles) and ``GM = 8`` are active."""
    _sweep(dev, entry, m, n, k, rows)


def test_fused_verify_counts_at_all_zero_expectation(dev):
    """K = 2240: the expectation is 0 everywhere, and a wrong row is still counted."""
    gpu, _ = _lib()
    m, n, k = 256, 256, 2240
    a, bt, ha, hbt = _filled(m, n, k)
    assert not ref.probe_expected_closed_form(m, n, k).any()
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    a[255, 2239] = float(ha[255, 2239] + 1)
    try:
        _fused_launch("probe", a, bt, m, n, k, None, counters.data_ptr())
    finally:
        a[255, 2239] = float(ha[255, 2239])
    assert counters.cpu().tolist()[gpu.ODH_SLOT_GEMM_ERR] == int((hbt[:, 2239] != 0).sum())


# ------------------------------------------------------------------ 3d. HBM kernels

HBM_N = [1, 63, 255, 256, 1023, 1024, 1025, 12305, 4096 * 1024 + 1]  # 16-byte elements
# 0xFFFFFFFC keeps b + 3 just below 2^32 at element 0; 0xFFFFFFFE makes b + 2 wrap to 0 there
HBM_SEEDS = [0, 0x9E3779B9, 0xFFFFFFFC, 0xFFFFFFFE]
HBM_BLOCKS = [1, 7, 4096]


@functools.lru_cache(maxsize=8)
def _pattern(n16, seed):
    return ref.pattern_words(n16, seed)  # shared between tests: never modified


def _as_i32(words):
    return torch.from_numpy(words.view(np.int32))


def _guarded(dev, words, fill=0x5C5C5C5C):
    """An int32 buffer of ``words`` payload words between two guards; returns (tensor, payload
    pointer = base + 256 bytes, 16-byte aligned)."""
    buf = torch.full((words + 2 * GUARD_WORDS,), fill, dtype=torch.int32, device=dev)
    buf[:GUARD_WORDS] = GUARD
    buf[GUARD_WORDS + words:] = GUARD
    ptr = buf.data_ptr() + 4 * GUARD_WORDS
    assert ptr % 16 == 0
    return buf, ptr


def _guards_intact(buf, words):
    return bool((buf[:GUARD_WORDS] == GUARD).all() and (buf[GUARD_WORDS + words:] == GUARD).all())


WRITERS = [("write", 0, 0), ("write", 1, 0)] + [("variant", v, b) for v in (1, 2, 3) for b in HBM_BLOCKS]


def _write(kind, arg, blocks, ptr, nbytes, seed):
    gpu, lib = _lib()
    if kind == "write":
        gpu._check(lib.odh_hbm_write(ptr, nbytes, seed, arg, _stream()))
    else:
        gpu._check(lib.odh_hbm_write_variant(ptr, nbytes, seed, arg, blocks, _stream()))


@pytest.mark.parametrize("seed", HBM_SEEDS)
@pytest.mark.parametrize("n16", HBM_N)
def test_hbm_write_matches_host_pattern(dev, n16, seed):
    """Every write kernel (plain and nontemporal, the three variants at 1, 7 and 4096
    workgroups) fills exactly ``n16`` elements with the host model's words; variant 3 writes
    the constant seed."""
    words = 4 * n16
    want = _as_i32(_pattern(n16, seed)).to(dev)
    want_const = torch.full((words,), seed - (1 << 32) if seed >> 31 else seed, dtype=torch.int32, device=dev)
    for kind, arg, blocks in WRITERS:
        buf, ptr = _guarded(dev, words)
        _write(kind, arg, blocks, ptr, 16 * n16, seed)
        payload = buf[GUARD_WORDS:GUARD_WORDS + words]
        expect = want_const if (kind, arg) == ("variant", 3) else want
        if not torch.equal(payload, expect):
            bad = (payload != expect).nonzero().flatten()
            pytest.fail(f"{kind} {arg} blocks={blocks} n={n16} seed={seed:#x}: {bad.numel()} wrong words, "
                        f"first at word {bad[0].item()}")
        assert _guards_intact(buf, words), (kind, arg, blocks)


@pytest.mark.parametrize("n16", [1, 1025])
def test_hbm_write_leaves_a_partial_tail_untouched(dev, n16):
    """``bytes = 16 n + 12``: the 12 bytes after the last whole element are not written."""
    seed = 0x9E3779B9
    words = 4 * n16 + 3
    want = torch.cat([_as_i32(_pattern(n16, seed)), torch.full((3,), 0x5C5C5C5C, dtype=torch.int32)]).to(dev)
    for kind, arg, blocks in WRITERS:
        if (kind, arg) == ("variant", 3):
            continue
        buf, ptr = _guarded(dev, words)
        _write(kind, arg, blocks, ptr, 16 * n16 + 12, seed)
        assert torch.equal(buf[GUARD_WORDS:GUARD_WORDS + words], want), (kind, arg, blocks)
        assert _guards_intact(buf, words)


CHECKERS = [("check", 0, 0)] + [("variant", v, b) for v in range(4) for b in HBM_BLOCKS]


def _check_launch(kind, arg, blocks, ptr, nbytes, seed, err_ptr):
    gpu, lib = _lib()
    if kind == "check":
        gpu._check(lib.odh_hbm_check(ptr, nbytes, seed, err_ptr, _stream()))
    else:
        gpu._check(lib.odh_hbm_check_variant(ptr, nbytes, seed, err_ptr, arg, blocks, _stream()))


def _flip_positions(words, seed):
    rng = np.random.default_rng(seed)
    pos = {0, 1 % words, words - 1, max(words - 2, 0)}
    pos.update(rng.choice(words, size=min(1000, words), replace=False).tolist())
    return np.array(sorted(pos), dtype=np.int64)


@pytest.mark.parametrize("seed", HBM_SEEDS)
@pytest.mark.parametrize("n16", HBM_N)
def test_hbm_check_counts_against_host_pattern(dev, n16, seed):
    """The pattern comes from the host model, not from the write kernel.  Each check kernel
    counts 0 on it, exactly the flipped words after single-bit flips, exactly the words that
    differ from the pattern of another seed, and adds to its counter."""
    words = 4 * n16
    host = _pattern(n16, seed)
    other = int((host != _pattern(n16, seed ^ 1)).sum())
    buf, ptr = _guarded(dev, words)
    buf[GUARD_WORDS:GUARD_WORDS + words] = _as_i32(host).to(dev)
    pos = _flip_positions(words, n16)
    flipped = host.copy()
    flipped[pos] ^= np.uint32(1) << (pos % 32).astype(np.uint32)
    fbuf, fptr = _guarded(dev, words)
    fbuf[GUARD_WORDS:GUARD_WORDS + words] = _as_i32(flipped).to(dev)
    # per checker: clean, flipped, other seed, accumulating twice — one u64 each
    err = torch.zeros((len(CHECKERS), 4), dtype=torch.int64, device=dev)
    for c, (kind, arg, blocks) in enumerate(CHECKERS):
        e = err.data_ptr() + 32 * c
        _check_launch(kind, arg, blocks, ptr, 16 * n16, seed, e)
        _check_launch(kind, arg, blocks, fptr, 16 * n16, seed, e + 8)
        _check_launch(kind, arg, blocks, ptr, 16 * n16, seed ^ 1, e + 16)
        _check_launch(kind, arg, blocks, fptr, 16 * n16, seed, e + 24)
        _check_launch(kind, arg, blocks, fptr, 16 * n16, seed, e + 24)
    got = err.cpu().tolist()
    for c, checker in enumerate(CHECKERS):
        assert got[c] == [0, len(pos), other, 2 * len(pos)], (checker, n16, hex(seed))
    assert _guards_intact(buf, words) and _guards_intact(fbuf, words)


def test_hbm_check_ignores_a_partial_tail(dev):
    n16, seed = 1025, 0x9E3779B9
    words = 4 * n16 + 3
    buf, ptr = _guarded(dev, words)
    buf[GUARD_WORDS:GUARD_WORDS + 4 * n16] = _as_i32(_pattern(n16, seed)).to(dev)
    err = torch.zeros((len(CHECKERS),), dtype=torch.int64, device=dev)
    for c, (kind, arg, blocks) in enumerate(CHECKERS):
        _check_launch(kind, arg, blocks, ptr, 16 * n16 + 12, seed, err.data_ptr() + 8 * c)
    assert err.cpu().tolist() == [0] * len(CHECKERS)


@pytest.mark.parametrize("n16", HBM_N[:-1])
def test_const_check_counts_exactly(dev, n16):
    gpu, lib = _lib()
    words = 4 * n16
    value = 0x3F800000  # the bits of a float, as in the all-reduce result check
    buf, ptr = _guarded(dev, words, fill=value)
    err = torch.zeros((3,), dtype=torch.int64, device=dev)
    gpu._check(lib.odh_const_check(ptr, 16 * n16, value, err.data_ptr(), _stream()))
    gpu._check(lib.odh_const_check(ptr, 16 * n16, value ^ 0x80000000, err.data_ptr() + 8, _stream()))
    pos = _flip_positions(words, 7 * n16)
    buf[GUARD_WORDS + torch.from_numpy(pos).to(dev)] = value + 1
    gpu._check(lib.odh_const_check(ptr, 16 * n16, value, err.data_ptr() + 16, _stream()))
    assert err.cpu().tolist() == [0, words, len(pos)]


def test_graph_replay_advances_the_seed_and_rewrites_the_pattern(dev):
    gpu, _ = _lib()
    p = gpu.GpuProbe(0, 256, 256, 64, hbm_bytes=1 << 20)
    try:
        seed = None
        for _ in range(3):
            r = p.run()
            assert r["ok"] and r["graph"], r
            seed = ref.lcg(0x1E3779B9 if seed is None else seed)
            assert int(p.seed_dev.item()) & 0xFFFFFFFF == seed
            assert torch.equal(p.hbm.cpu(), _as_i32(ref.pattern_words((1 << 20) // 16, seed)))
    finally:
        p.close()


# ------------------------------------------------------------------ 3e. busy kernel


@pytest.mark.parametrize("blocks", [1, 3])
def test_busy_output_matches_mfma_layout_model(dev, blocks):
    gpu, lib = _lib()
    per_lane = torch.from_numpy(ref.busy_expected().astype(np.float32))
    iters = [0, 1, 3, 1000]
    out = torch.full((len(iters), blocks * 256), float("nan"), device=dev)
    for x, it in enumerate(iters):
        gpu._check(lib.odh_busy(out[x].data_ptr(), blocks, it, _stream()))
    got = out.cpu()
    for x, it in enumerate(iters):
        want = (per_lane * it).repeat(blocks * 4)  # values stay far below 2^24: exact
        assert torch.equal(got[x], want), (it, got[x][:64].tolist(), want[:64].tolist())


# ------------------------------------------------------------------ 3f. argument guards


def test_argument_guards_return_invalid_value_and_launch_nothing(dev):
    """Every call below is refused on the host side; the sentinel-filled outputs stay as they were."""
    gpu, lib = _lib()
    s = _stream()
    buf = torch.full((1024,), 0x5C5C5C5C, dtype=torch.int32, device=dev)
    err = torch.full((4,), -7, dtype=torch.int64, device=dev)
    c = torch.full((256, 256), float("nan"), device=dev)
    a = torch.zeros((256, 256), dtype=torch.bfloat16, device=dev)
    cnt = torch.full((gpu.ODH_NCOUNT,), -7, dtype=torch.int32, device=dev)
    tile_xcd = torch.full((16,), -1, dtype=torch.int32, device=dev)
    b, e, cp = buf.data_ptr(), err.data_ptr(), cnt.data_ptr()
    xb, ge, ex = (cp + 4 * slot for slot in (gpu.ODH_SLOT_XCD_BLOCKS, gpu.ODH_SLOT_GEMM_ERR, gpu.ODH_SLOT_ERR_XCD))
    ap, cpt, tx = a.data_ptr(), c.data_ptr(), tile_xcd.data_ptr()
    calls = {
        "write bytes<16": lambda: lib.odh_hbm_write(b, 15, 1, 0, s),
        "write nt bytes<16": lambda: lib.odh_hbm_write(b, 0, 1, 1, s),
        "write variant bytes<16": lambda: lib.odh_hbm_write_variant(b, 15, 1, 2, 4, s),
        "write variant blocks=0": lambda: lib.odh_hbm_write_variant(b, 4096, 1, 1, 0, s),
        "write variant blocks<0": lambda: lib.odh_hbm_write_variant(b, 4096, 1, 3, -1, s),
        "check bytes<16": lambda: lib.odh_hbm_check(b, 15, 1, e, s),
        "check variant bytes<16": lambda: lib.odh_hbm_check_variant(b, 15, 1, e, 0, 4, s),
        "check variant blocks=0": lambda: lib.odh_hbm_check_variant(b, 4096, 1, e, 0, 0, s),
        "check variant 4": lambda: lib.odh_hbm_check_variant(b, 4096, 1, e, 4, 4, s),
        "check variant -1": lambda: lib.odh_hbm_check_variant(b, 4096, 1, e, -1, 4, s),
        "const bytes%16": lambda: lib.odh_const_check(b, 4096 + 4, 1, e, s),
        "const bytes<16": lambda: lib.odh_const_check(b, 12, 1, e, s),
        "busy blocks=0": lambda: lib.odh_busy(cpt, 0, 1, s),
        "busy iters<0": lambda: lib.odh_busy(cpt, 1, -1, s),
        "fused NULL err_total": lambda: lib.odh_probe_gemm_verify(ap, ap, 256, 256, 256, tx, xb, None, ex, s),
        "2buf NULL err_total": lambda: lib.odh_probe_gemm_verify_2buf(ap, ap, 256, 256, 256, tx, xb, None, ex, s),
        "deep NULL err_total": lambda: lib.odh_probe_gemm_verify_deep(ap, ap, 256, 256, 256, tx, xb, None, ex, 0, s),
        "deep variant 8": lambda: lib.odh_probe_gemm_verify_deep(ap, ap, 256, 256, 256, tx, xb, ge, ex, 8, s),
        "deep variant -1": lambda: lib.odh_probe_gemm_verify_deep(ap, ap, 256, 256, 256, tx, xb, ge, ex, -1, s),
        "fill M%128": lambda: lib.odh_probe_fill(ap, ap, 200, 256, 256, s),
        "verify K%32": lambda: lib.odh_probe_verify(cpt, 256, 256, 48, tx, ge, ex, s),
    }
    # shapes the 128² tile divides but the 256² tile does not, for the fused entry points and the
    # 256² store kernels; shapes no tile divides, for every GEMM entry point
    for m, n, k in ((128, 256, 256), (256, 128, 256), (256, 256, 32), (256, 256, 0)):
        calls[f"fused {m},{n},{k}"] = lambda m=m, n=n, k=k: lib.odh_probe_gemm_verify(ap, ap, m, n, k, tx, xb, ge, ex,
                                                                                      s)
        calls[f"2buf {m},{n},{k}"] = lambda m=m, n=n, k=k: lib.odh_probe_gemm_verify_2buf(ap, ap, m, n, k, tx, xb, ge,
                                                                                         ex, s)
        for v in (0, 5, 6):
            calls[f"deep{v} {m},{n},{k}"] = lambda m=m, n=n, k=k, v=v: lib.odh_probe_gemm_verify_deep(
                ap, ap, m, n, k, tx, xb, ge, ex, v, s)
        for v in range(4):
            calls[f"store v{v} {m},{n},{k}"] = lambda m=m, n=n, k=k, v=v: lib.odh_gemm_bf16_256_variant(
                ap, ap, cpt, m, n, k, v, s)
    for m, n, k in ((100, 256, 256), (256, 200, 256), (256, 256, 48), (0, 256, 256), (256, 256, -32)):
        calls[f"gemm {m},{n},{k}"] = lambda m=m, n=n, k=k: lib.odh_gemm_bf16(ap, ap, cpt, m, n, k, tx, xb, s)
        calls[f"gemm128 {m},{n},{k}"] = lambda m=m, n=n, k=k: lib.odh_gemm_bf16_128(ap, ap, cpt, m, n, k, tx, xb, s)
        calls[f"store v2 {m},{n},{k}"] = lambda m=m, n=n, k=k: lib.odh_gemm_bf16_256_variant(ap, ap, cpt, m, n, k, 2, s)
        assert lib.odh_gemm_tiles(m, n, k) == 0 and not lib.odh_gemm_shape_ok(m, n, k)
    for name, call in calls.items():
        assert call() != 0, f"{name}: accepted"
    torch.cuda.synchronize()
    assert (buf == 0x5C5C5C5C).all() and (err == -7).all() and (cnt == -7).all() and (tile_xcd == -1).all()
    assert torch.isnan(c).all()
