"""The 2:4 structured-sparsity probe kernels on a real MI355X against a host product: ``v_smfmac_*`` in
bf16, f16, i8, fp8 and bf8 through ``odh_sparse_gemm``, ``odh_sparse_fill``,
``odh_sparse_probe_gemm_verify`` and ``odh-gpu-probe --sparse``.

Everything is bit-exact.  Operands are integers the format holds exactly; each case checks on the
CPU that ``sum_k |a| |b|`` stays below ``2^24`` (fp32 accumulation) or ``2^31`` (i8), so every
partial sum is an integer the accumulator holds and the result is exact in any summation order.
The tests corrupt data only; every pointer handed to a kernel comes from a torch allocation at
least as large as the shape implies.
"""

import functools
import json

import numpy as np
import pytest

import sparse_reference as sp
from probe_gpu import _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = sp.FORMATS
# random operands: integers every one of which the format holds exactly (fp8 has 4 significant
# bits, bf8 3); i8 over its full range
RANDOM = {"bf16": (-15, 15), "f16": (-15, 15), "i8": (-128, 127), "fp8": (-15, 15), "bf8": (-7, 7)}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.int8, "fp8": torch.float8_e4m3fn,
               "bf8": torch.float8_e5m2}
VERIFY_K = 640  # the smallest multiple of 128 at which no class expects 0


def _t(fmt, ints, dev):
    """Integers the format holds exactly as a tensor of the format on the GPU."""
    if fmt == "i8":
        return torch.from_numpy(ints.astype(np.int8)).to(dev)
    t = torch.from_numpy(ints.astype(np.float32)).to(TORCH_DTYPE[fmt])
    assert np.array_equal(t.float().numpy(), ints.astype(np.float32))  # exact
    return t.to(dev)


def _meta(meta, dev):
    return torch.from_numpy(np.ascontiguousarray(meta)).to(dev)


def _out_dtype(fmt):
    return torch.int32 if fmt == "i8" else torch.float32


def _assert_exact(what, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{what}: {len(bad)} wrong elements in {len(np.unique(bad[:, 0]))} rows and "
                    f"{len(np.unique(bad[:, 1]))} columns, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


# ------------------------------------------------------------------ store kernel


@functools.lru_cache(maxsize=None)
def _random_case(fmt, m, n, k):
    """Seeded random integer operands: compressed A and Bt drawn independently, metadata random over
    the six valid nibbles, and their exact int64 product."""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + 7 * FORMATS.index(fmt))
    lo, hi = RANDOM[fmt]
    ac = rng.integers(lo, hi + 1, size=(m, k // 2), dtype=np.int64)
    bt = rng.integers(lo, hi + 1, size=(n, k), dtype=np.int64)
    meta = sp.pack_meta(rng.choice(sp.VALID_NIBBLES, size=(m, k // 4)))
    a = sp.decompress(ac, meta)
    want = a @ bt.T
    # exact in any summation order: every partial sum stays below the accumulator's exact range
    assert (np.abs(a) @ np.abs(bt).T).max() < sp.EXACT_BELOW[fmt]
    assert not np.array_equal(want[:min(m, n), :min(m, n)], want[:min(m, n), :min(m, n)].T)
    return ac, meta, bt, want


def _exact_store(dev, fmt, m, n, k):
    ac, meta, bt, want = _random_case(fmt, m, n, k)
    c = torch.full((m, n), -77, dtype=_out_dtype(fmt), device=dev)
    _gpu().sparse_gemm(fmt, _t(fmt, ac, dev), _meta(meta, dev), _t(fmt, bt, dev), out=c)
    _assert_exact(f"{fmt} {m}x{n}x{k}", c.cpu().numpy().astype(np.int64), want)


# fewer than, equal to and more than the two stages in flight and the three ring slots: ring fill,
# wrap and drain; then a long K of 64 stages
K_STAGES = [1, 2, 3, 4, 5, 7, 64]
# one stage; non-square grids whose workgroup counts exercise the XCD remap's remainders
GRIDS = [(512, 1024), (768, 768), (256, 2816)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stages", K_STAGES)
def test_sparse_gemm_exact_over_k(dev, fmt, stages):
    _exact_store(dev, fmt, 256, 256, stages * sp.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", GRIDS)
def test_sparse_gemm_exact_over_grids(dev, fmt, m, n):
    _exact_store(dev, fmt, m, n, sp.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_sparse_gemm_exact_over_tiles_and_stages(dev, fmt):
    """2 × 3 tiles at 3 stages: operand and metadata addresses with a tile offset and ``kt > 0``."""
    _exact_store(dev, fmt, 512, 768, 3 * sp.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_sparse_lane_map(dev, fmt):
    """One launch: every row has one non-zero kept element, every kept slot of a stage and every
    position a slot can select occur, and Bt identifies k: each output is the one value the host
    model names.  A wrong operand, index or selector map fails here."""
    ac, meta, bt, want = sp.lanemap_case(fmt)
    if fmt in ("fp8", "bf8"):
        tb = torch.from_numpy(bt).view(TORCH_DTYPE[fmt]).to(dev)  # codes
    else:
        tb = _t(fmt, bt, dev)
    c = _gpu().sparse_gemm(fmt, _t(fmt, ac, dev), _meta(meta, dev), tb)
    _assert_exact(f"{fmt} lane map", c.cpu().numpy().astype(np.float64), want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_sparse_gemm_of_a_pruned_matrix(dev, fmt):
    """``sparse_compress(prune=True)`` of random integers on the GPU, then ``sparse_gemm``: the product
    with the pruned dense matrix, which keeps the two largest magnitudes of every group."""
    gpu = _gpu()
    m, n, k = 256, 256, 2 * sp.STAGE[fmt]
    rng = np.random.default_rng(2400 + FORMATS.index(fmt))
    lo, hi = RANDOM[fmt]
    a = rng.integers(lo, hi + 1, size=(m, k), dtype=np.int64)
    bt = rng.integers(lo, hi + 1, size=(n, k), dtype=np.int64)
    ac, meta = gpu.sparse_compress(_t(fmt, a, dev), prune=True)
    assert ac.device == meta.device == dev and ac.dtype == TORCH_DTYPE[fmt]
    hac, hmeta = sp.compress(a, prune=True)
    assert np.array_equal(meta.cpu().numpy(), hmeta)
    pruned = sp.decompress(hac, hmeta)
    g = np.abs(pruned.reshape(m, k // 4, 4))
    full = np.sort(np.abs(a.reshape(m, k // 4, 4)), axis=-1)
    assert np.array_equal(np.sort(g, axis=-1)[..., 2:], full[..., 2:]) and ((g != 0).sum(-1) <= 2).all()
    back = gpu.sparse_decompress(ac, meta)
    assert np.array_equal(back.cpu().float().numpy() if fmt != "i8" else back.cpu().numpy(), pruned)
    c = gpu.sparse_gemm(fmt, ac, meta, _t(fmt, bt, dev))
    _assert_exact(f"{fmt} pruned", c.cpu().numpy().astype(np.int64), pruned @ bt.T)


# ------------------------------------------------------------------ entry points refuse


def test_sparse_entry_points_check_before_launch(dev):
    gpu = _gpu()
    fmt = "f16"
    ac, meta, bt, _ = _random_case(fmt, 256, 256, 128)
    ta, tm, tb = _t(fmt, ac, dev), _meta(meta, dev), _t(fmt, bt, dev)
    for bad in ("f32", "fp4", 5, -1):
        with pytest.raises(ValueError):
            gpu.sparse_gemm(bad, ta, tm, tb)
    with pytest.raises(TypeError):
        gpu.sparse_gemm("bf16", ta, tm, tb)
    with pytest.raises(TypeError):
        gpu.sparse_gemm(fmt, ta, tm.to(torch.int8), tb)
    with pytest.raises(ValueError):
        gpu.sparse_gemm(fmt, ta, tm, tb[:, :64].contiguous())  # K of Ac and Bt differ
    with pytest.raises(ValueError):
        gpu.sparse_gemm(fmt, ta[:, :16].contiguous(), tm[:, :4].contiguous(), tb[:, :32].contiguous())  # half a stage
    with pytest.raises(ValueError):
        gpu.sparse_gemm(fmt, ta[:128].contiguous(), tm[:128].contiguous(), tb)
    with pytest.raises(ValueError):
        gpu.sparse_gemm(fmt, ta, tm[:, :8].contiguous(), tb)
    with pytest.raises(ValueError):
        gpu.sparse_gemm(fmt, ta.cpu(), tm, tb)
    with pytest.raises(ValueError):
        gpu.sparse_gemm(fmt, ta, tm, tb, out=torch.empty((256, 256), dtype=torch.int32, device=dev))
    table = torch.zeros(gpu.SPARSE_TABLE, dtype=torch.int32, device=dev)
    for fn in (gpu.sparse_fill, gpu.sparse_verify):
        with pytest.raises(ValueError):
            fn(fmt, ta, tm, tb, table)  # K = 128 has a class that expects 0
    with pytest.raises(ValueError):
        gpu.sparse_probe(0, fmt, 256, 256, 128)
    with pytest.raises(ValueError):
        gpu.sparse_probe(0, "i8", 256, 256, 320)  # no zero class, but no whole number of i8 stages


def test_sparse_c_abi_refuses_before_launch(dev):
    """The library's own checks, below the Python ones: ``hipErrorInvalidValue`` and no launch.
    The buffers are large enough for every shape tried here."""
    gpu = _gpu()
    lib = gpu.load_library()
    invalid = 1  # hipErrorInvalidValue
    ac = torch.zeros((512, 640), dtype=torch.int16, device=dev)
    bt = torch.zeros((512, 1280), dtype=torch.int16, device=dev)
    meta = torch.zeros((512, 160), dtype=torch.uint8, device=dev)
    c = torch.zeros((512, 512), dtype=torch.int32, device=dev)
    table = torch.zeros(gpu.SPARSE_TABLE, dtype=torch.int32, device=dev)
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pa, pm, pb, pc, pt, pk = (x.data_ptr() for x in (ac, meta, bt, c, table, counters))
    bf16, i8 = gpu.ODH_SP_BF16, gpu.ODH_SP_I8
    for args in ((5, pa, pm, pb, 256, 256, 640), (-1, pa, pm, pb, 256, 256, 640),  # unknown formats
                 (bf16, pa, pm, pb, 128, 256, 640), (bf16, pa, pm, pb, 256, 384, 640), (bf16, pa, pm, pb, 256, 256, 32),
                 (i8, pa, pm, pb, 256, 256, 64), (i8, pa, pm, pb, 256, 256, 320), (bf16, pa, pm, pb, 256, 256, 0),
                 (bf16, pa, pm, pb, 0, 256, 640), (bf16, None, pm, pb, 256, 256, 640),
                 (bf16, pa, None, pb, 256, 256, 640), (bf16, pa, pm, None, 256, 256, 640),
                 (bf16, pa + 8, pm, pb, 256, 256, 640), (bf16, pa, pm, pb + 4, 256, 256, 640),  # not 16-byte aligned
                 (bf16, pa, pm + 2, pb, 256, 256, 640)):  # metadata not 4-byte aligned
        fmt, xa, xm, xb, m, n, k = args
        assert lib.odh_sparse_gemm(fmt, xa, xm, xb, pc, m, n, k, s) == invalid, args
        assert lib.odh_sparse_fill(fmt, xa, xm, xb, pt, m, n, k, s) == invalid, args
        assert lib.odh_sparse_probe_gemm_verify(fmt, xa, xm, xb, pt, m, n, k, None, pk, s) == invalid, args
    assert lib.odh_sparse_gemm(bf16, pa, pm, pb, None, 256, 256, 640, s) == invalid
    assert lib.odh_sparse_fill(bf16, pa, pm, pb, None, 256, 256, 640, s) == invalid
    assert lib.odh_sparse_probe_gemm_verify(bf16, pa, pm, pb, None, 256, 256, 640, None, pk, s) == invalid
    assert lib.odh_sparse_probe_gemm_verify(bf16, pa, pm, pb, pt, 256, 256, 640, None, None, s) == invalid
    for k in (64, 128, 256, 768):  # a class expects 0: fill and check refuse
        assert sp.zero_classes(k) > 0
        assert lib.odh_sparse_fill(bf16, pa, pm, pb, pt, 256, 256, k, s) == invalid, k
        assert lib.odh_sparse_probe_gemm_verify(bf16, pa, pm, pb, pt, 256, 256, k, None, pk, s) == invalid, k
    torch.cuda.synchronize(dev)
    for x in (ac, bt, meta, c, table, counters):
        assert int(x.to(torch.int64).abs().sum()) == 0


# ------------------------------------------------------------------ fill and fused verify


def _filled(dev, fmt, m, n, k):
    gpu = _gpu()
    ac = torch.zeros((m, k // 2), dtype=TORCH_DTYPE[fmt], device=dev)
    meta = torch.full((m, k // 8), 0x77, dtype=torch.uint8, device=dev)
    bt = torch.zeros((n, k), dtype=TORCH_DTYPE[fmt], device=dev)
    table = torch.full(gpu.SPARSE_TABLE, -1, dtype=torch.int32, device=dev)
    gpu.sparse_fill(fmt, ac, meta, bt, table)
    return ac, meta, bt, table


def _ints(fmt, t):
    return t.cpu().numpy().astype(np.int64) if fmt == "i8" else t.cpu().float().numpy().astype(np.int64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_sparse_fill_matches_the_model(dev, fmt):
    m, n, k = 256, 512, VERIFY_K
    ac, meta, bt, table = _filled(dev, fmt, m, n, k)
    hac, hmeta, hbt = sp.fill(fmt, m, n, k)
    assert np.array_equal(meta.cpu().numpy(), hmeta)
    assert set(np.unique(sp.unpack_meta(hmeta)).tolist()) == set(sp.VALID_NIBBLES)
    assert np.array_equal(_ints(fmt, ac), hac) and np.array_equal(_ints(fmt, bt), hbt)
    if fmt in ("fp8", "bf8"):  # the codes themselves: the model's encoder, and no -0
        code = sp.fp8_code if fmt == "fp8" else sp.bf8_code
        assert np.array_equal(ac.view(torch.uint8).cpu().numpy(), code(hac))
        assert np.array_equal(bt.view(torch.uint8).cpu().numpy(), code(hbt))
    assert np.array_equal(table.cpu().numpy().astype(np.int64), sp.table(k))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", [(256, 256), (512, 768)])
def test_sparse_verify_clean(dev, fmt, m, n):
    r = _gpu().sparse_verify(fmt, *_filled(dev, fmt, m, n, VERIFY_K))
    assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert sum(r["xcd_blocks"]) == (m // 256) * (n // 256), r


def _verify_raw(dev, fmt, ac, meta, bt, table, m, n, k):
    """The fused check with a tile map of its own: total, per-XCD counts, and the XCD of every tile."""
    gpu = _gpu()
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    tile_xcd = torch.full(((m // 256) * (n // 256),), -1, dtype=torch.int32, device=dev)
    rc = gpu.load_library().odh_sparse_probe_gemm_verify(
        gpu.SPARSE_FORMATS[fmt], ac.data_ptr(), meta.data_ptr(), bt.data_ptr(), table.data_ptr(), m, n, k,
        tile_xcd.data_ptr(), counters.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    h = counters.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return (int(h[gpu.ODH_SLOT_GEMM_ERR]), h[gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.ODH_N_XCD],
            tile_xcd.cpu().numpy())


def _assert_counts(dev, fmt, tensors, host, m, n, k, what):
    """The check's total and per-XCD attribution against the host model's mismatches."""
    hac, hmeta, hbt = host
    wrong = sp.mismatches(fmt, hac, hmeta, hbt, k)
    want = int(wrong.sum())
    assert want > 0, what
    total, err_xcd, tile_xcd = _verify_raw(dev, fmt, *tensors, m, n, k)
    want_xcd = np.zeros(8, dtype=np.int64)
    np.add.at(want_xcd, tile_xcd, sp.per_tile(wrong).reshape(-1))
    assert total == want and np.array_equal(err_xcd, want_xcd), (what, total, want, err_xcd, want_xcd)
    return wrong


# (row, kept slot) of a changed compressed value: first and last row and slot, and a row of every
# wave row of the tile (wave rows are 128 rows; fragments 32)
VALUE_CASES = [(0, 0), (511, VERIFY_K // 2 - 1), (130, 77), (300, 161)]
# (row, group, replacement pair): each of the six pairs, first and last row and group
NIBBLE_CASES = [(0, 0, (0, 1)), (511, VERIFY_K // 4 - 1, (2, 3)), (129, 7, (0, 2)), (255, 80, (1, 2)),
                (256, 33, (1, 3)), (400, 101, (0, 3))]
# (column, k) of a changed B element: first and last column and k, and a column of every wave column
B_CASES = [(0, 0), (767, VERIFY_K - 1), (70, 321), (130, 5), (200, 638), (500, 300)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_sparse_verify_counts_changed_operands(dev, fmt):
    """One compressed value, one metadata nibble, one B element changed at a time (and put back):
    the count and its per-XCD attribution are the host model's."""
    m, n, k = 512, 768, VERIFY_K
    ac, meta, bt, table = _filled(dev, fmt, m, n, k)
    hac, hmeta, hbt = sp.fill(fmt, m, n, k)
    tensors = (ac, meta, bt, table)
    mul_a, mul_b = sp.MUL[fmt]
    for r, s in VALUE_CASES:
        old = hac[r, s]
        new = (1 if old != mul_a else 2) * mul_a
        h2 = hac.copy()
        h2[r, s] = new
        keep = ac[r, s:s + 1].clone()
        ac[r, s:s + 1].copy_(_t(fmt, np.array([new]), dev))
        wrong = _assert_counts(dev, fmt, tensors, (h2, hmeta, hbt), m, n, k, ("value", r, s))
        assert not np.delete(wrong, r, axis=0).any()
        ac[r, s:s + 1].copy_(keep)
    for r, g, (p0, p1) in NIBBLE_CASES:
        nib = sp.unpack_meta(hmeta)
        new = p0 | p1 << 2
        if nib[r, g] == new:  # the fill has this pair here: the next group of the row has another
            g += 1
        assert nib[r, g] != new
        nib[r, g] = new
        m2 = sp.pack_meta(nib)
        keep = meta[r, g // 2:g // 2 + 1].clone()
        meta[r, g // 2:g // 2 + 1].copy_(torch.from_numpy(m2[r, g // 2:g // 2 + 1]))
        wrong = _assert_counts(dev, fmt, tensors, (hac, m2, hbt), m, n, k, ("nibble", r, g, new))
        assert not np.delete(wrong, r, axis=0).any()
        meta[r, g // 2:g // 2 + 1].copy_(keep)
    for j, kk in B_CASES:
        old = hbt[j, kk]
        new = (1 if old != mul_b else 2) * mul_b
        b2 = hbt.copy()
        b2[j, kk] = new
        keep = bt[j, kk:kk + 1].clone()
        bt[j, kk:kk + 1].copy_(_t(fmt, np.array([new]), dev))
        wrong = _assert_counts(dev, fmt, tensors, (hac, hmeta, b2), m, n, k, ("b", j, kk))
        assert not np.delete(wrong, j, axis=1).any()
        bt[j, kk:kk + 1].copy_(keep)
    total, err_xcd, _ = _verify_raw(dev, fmt, *tensors, m, n, k)  # everything put back
    assert total == 0 and not err_xcd.any()


def test_sparse_probe_reports_the_check(dev):
    for fmt in FORMATS:
        r = _gpu().sparse_probe(0, fmt, 512, 512, VERIFY_K)
        assert set(r) == {"errors", "err_xcd", "xcd_blocks", "ms", "tflops"}
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == 4 and r["ms"] > 0


# ------------------------------------------------------------------ the program


ALL = "bf16,f16,i8,fp8,bf8"


def test_sparse_program_passes_with_every_step_under_the_message_limit():
    rc, res, r = _run_probe("--mx", "fp8,fp4,bf8,fp6,bf6", "--dtypes", "f16,i8", "--fp", "f32,f64", "--sparse", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["sparse"]) == FORMATS
    for f in res["sparse"].values():
        assert f["ok"] is True and f["errors"] == 0 and f["ms"] > 0 and f["host_ms"] > 0, res["sparse"]
    keys = list(res)
    assert keys.index("mx") < keys.index("dtypes") < keys.index("fp") < keys.index("sparse")
    assert keys[-3:] == ["sparse", "setup_ms", "timings_ms"]
    t = list(res["timings_ms"])
    assert t.index("mx") < t.index("dtypes") < t.index("fp") < t.index("sparse") < t.index("total")
    assert res["timings_ms"]["sparse"] > 0
    rccl = ',"rccl":{"ranks":8,"ok":false,"errors":18446744073709551615,"mib":128,"load_ms":99999.99,' \
           '"init_ms":99999.99,"allreduce_ms":99999.9999,"busbw_gbps":99999.9}'
    line = r.stdout.strip().splitlines()[-1]
    print("verdict bytes:", len(line), "sparse:", json.dumps(res["sparse"]), json.dumps(res["timings_ms"]))
    assert len(line) + len(rccl) < 4096


def test_sparse_program_alone_and_without():
    rc, res, r = _run_probe("--sparse", "i8,bf16")
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["sparse"]) == ["i8", "bf16"] and "mx" not in res and "fp" not in res
    rc, res, r = _run_probe()
    assert rc == 0 and res["ok"] and "sparse" not in res and "sparse" not in res["timings_ms"], r.stdout


def test_sparse_program_fails_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--sparse", ALL, "--inject-fault", "sparse")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    # the nibble of row 0, group 0 becomes the pair (0,1): the host model's count
    m, n, k = 256, 4096, 1024
    hac, hmeta, hbt = sp.fill("bf16", m, n, k)
    nib = sp.unpack_meta(hmeta)
    assert nib[0, 0] == 12 and hmeta[0, 0] == 0xEC
    nib[0, 0] = 4
    wrong = sp.mismatches("bf16", hac, sp.pack_meta(nib), hbt, k)
    want = int(wrong.sum())
    assert want == n and wrong[0].all()
    assert res["ok"] is False
    for fmt in FORMATS:
        assert res["sparse"][fmt]["ok"] is False and res["sparse"][fmt]["errors"] == want, res["sparse"]
    assert "GPU 0" in res["error"] and "bf16" in res["error"] and "sparse GEMM" in res["error"], res["error"]
    assert "XCD" in res["error"]
    d = res["results"][0]
    assert d["ok"] is True and d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
