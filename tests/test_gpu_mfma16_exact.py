"""The 16×16 matrix-core kernels on a real MI355X against the host model (``mfma16_reference.py``):
``v_mfma_f32_16x16x32_bf16`` / ``_f16``, ``v_mfma_i32_16x16x64_i8`` and ``v_mfma_scale_f32_16x16x128_f8f6f4`` (fp8,
fp4) through ``odh_m16_one``, ``odh_m16_gemm``, ``odh_m16_probe_gemm_verify`` and ``odh-gpu-probe --mfma16``.

Everything is bit-exact.  Operands are integers (times powers of two for the scaled formats); each case checks on
the CPU that ``sum_k |a| |b|`` stays below ``2^24`` (fp32 accumulators) or ``2^31`` (i8), so the result is exact in
any summation order.  The tests corrupt data only; every pointer handed to a kernel comes from a torch allocation of
exactly the size the shape implies.
"""

import functools
import json

import numpy as np
import pytest

import mfma16_reference as m16
import mx_reference as mx
import probe_reference as ref
from probe_gpu import _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = list(m16.FORMATS)
TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.int8, "fp8": torch.uint8, "fp4": torch.uint8}
I8_MUL_A, I8_MUL_B = 25, 41
UNIT = 0x7F7F7F7F  # 1.0 in every byte of a scale VGPR


# ------------------------------------------------------------------ one instruction


def _run_cases(dev, fmt, a, b, sa=None, sb=None, opsel_a=0, opsel_b=0):
    """``odh_m16_one`` once per case, each on tensors of its own; ``[cases, 64, 4]`` values."""
    gpu = _gpu()
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    scaled = fmt in m16.SCALED
    if scaled:
        tsa, tsb = torch.from_numpy(sa).to(dev), torch.from_numpy(sb).to(dev)
    out = []
    for i in range(a.shape[0]):
        s = (tsa[i].clone(), tsb[i].clone()) if scaled else (None, None)
        out.append(gpu.m16_one(fmt, ta[i].clone(), tb[i].clone(), *s, opsel_a=opsel_a, opsel_b=opsel_b))
    return m16.result_values(fmt, torch.stack(out).cpu().numpy())


def _assert_cases(what, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        c, lane, r = bad[0]
        pytest.fail(f"{what}: {len(np.unique(bad[:, 0]))} of {got.shape[0]} cases differ, first case {c} lane {lane} "
                    f"register {r}: {got[c, lane, r]!r} != {want[c, lane, r]!r}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_instruction_on_random_integers(dev, fmt):
    """Random integer elements, and for fp8 and fp4 a random scale 2^-2 .. 2^2 in every byte of every lane's scale
    VGPR, under every pair of ``opsel``."""
    rng = np.random.default_rng(31 + m16.CODES[fmt])
    pairs = [(oa, ob) for oa in range(4) for ob in range(4)] if fmt in m16.SCALED else [(0, 0)] * 4
    for oa, ob in pairs:
        lo, hi = (-128, 128) if fmt == "i8" else (-3, 4)
        a, b = m16.random_registers(fmt, rng, lo, hi), m16.random_registers(fmt, rng, lo, hi)
        sa = rng.integers(125, 130, size=(64, 4)).astype(np.uint8).view(np.int32).reshape(64)
        sb = rng.integers(125, 130, size=(64, 4)).astype(np.uint8).view(np.int32).reshape(64)
        want, mag = m16.one(fmt, a, b, sa, sb, oa, ob)
        assert mag.max() * 16 < m16.EXACT_BELOW[fmt]  # × 16: the scales' products are multiples of 2^-4
        got = _run_cases(dev, fmt, a[None], b[None], sa[None], sb[None], oa, ob)
        _assert_cases(f"{fmt} opsel {oa},{ob}", got, want[None])
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_hot_at_every_lane_and_element(dev, fmt, side):
    """A single 1 at every (lane, element) of one side against a random integer operand on the other: the lane's
    row or column, the element's k, and the result register of every product."""
    a, b = m16.one_hot_family(fmt, side)
    unit = np.full((a.shape[0], 64), UNIT, dtype=np.int32)
    want, mag = m16.one(fmt, a, b, unit, unit)
    assert mag.max() < m16.EXACT_BELOW[fmt]
    # no case is vacuous, and the random side tells any two k apart
    assert (np.abs(want).reshape(want.shape[0], -1).max(axis=1) > 0).all()
    other = m16.decode(fmt, m16.elements(fmt, (b if side == "a" else a)[0]))
    cols = m16.operand(fmt, (b if side == "a" else a)[0], unit[0]).T  # [k][16]
    assert len({tuple(c) for c in cols.tolist()}) == m16.STAGE[fmt] and other.shape == (64, m16.ELEMS[fmt])
    _assert_cases(f"{fmt} one-hot {side}", _run_cases(dev, fmt, a, b, unit, unit), want)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("fmt", m16.SCALED)
def test_a_distinct_scale_in_every_lane_and_byte(dev, fmt, side):
    """A single 1.0 at every eighth element of every lane (both register halves of an fp8 lane) against all ones,
    with a scale byte of its own in every lane and byte position of that side's scale VGPRs, ``opsel`` 0-3: each
    output of the hot row or column is 2^(the routed byte - 127), which names the lane and byte it came from."""
    for opsel in range(4):
        for wrap in m16.SCALE_WRAPS:
            a, b, sa, sb = m16.scale_family(fmt, side, opsel, wrap)
            oa, ob = (opsel, 0) if side == "a" else (0, opsel)
            want, _ = m16.one(fmt, a, b, sa, sb, oa, ob)  # one product per output: exact at any scale
            nz = want.reshape(want.shape[0], -1)
            assert ((nz != 0).sum(axis=1) == 16).all() and np.isfinite(want).all()
            _assert_cases(f"{fmt} scales of {side}, opsel {opsel}, wrap {wrap}",
                          _run_cases(dev, fmt, a, b, sa, sb, oa, ob), want)


# ------------------------------------------------------------------ store kernel


@functools.lru_cache(maxsize=None)
def _random_case(fmt, m, n, k):
    """Seeded random operands in the public layout, scales for fp8 and fp4, and their exact product."""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + m16.CODES[fmt])
    if fmt in m16.SCALED:
        code = m16.MX_CODE[fmt]
        va, vb = rng.integers(-3, 4, size=(m, k)), rng.integers(-3, 4, size=(n, k))
        lut = mx.unpack(code, mx.encode(code, np.arange(-4.0, 4.0)[None]))[0]  # the codes of -4 .. 3 (fp8: 8 bytes)
        assert np.array_equal(mx.decode_codes(code, lut), np.arange(-4.0, 4.0))
        a, bt = mx.pack(code, lut[va + 4]), mx.pack(code, lut[vb + 4])
        sa = rng.integers(126, 129, size=(m, k // 32)).astype(np.uint8)
        sbt = rng.integers(126, 129, size=(n, k // 32)).astype(np.uint8)
        want = mx.product(code, a, bt, sa, sbt)
        mag = np.abs(mx.scaled(code, a, sa)) @ np.abs(mx.scaled(code, bt, sbt)).T
        assert mag.max() * 4 < m16.EXACT_BELOW[fmt]  # multiples of 2^-2
        return (a, bt, sa, sbt), want
    lo, hi = (-128, 128) if fmt == "i8" else (-8, 9)
    va = rng.integers(lo, hi, size=(m, k), dtype=np.int64)
    vb = rng.integers(lo, hi, size=(n, k), dtype=np.int64)
    if fmt == "i8":
        va[0, 0], vb[0, 0] = -128, -128
    assert (np.abs(va) @ np.abs(vb).T).max() < m16.EXACT_BELOW[fmt]
    return (va, vb), (va @ vb.T).astype(np.float64)


def _to_dev(dev, fmt, arrays):
    if fmt in m16.SCALED:
        return [torch.from_numpy(x).to(dev) for x in arrays]
    return [torch.from_numpy(x.astype(np.float32 if fmt != "i8" else np.int8)).to(dev).to(TORCH_DTYPE[fmt])
            for x in arrays]


def _exact_store(dev, fmt, m, n, k):
    gpu = _gpu()
    arrays, want = _random_case(fmt, m, n, k)
    ts = _to_dev(dev, fmt, arrays)
    if fmt == "i8":
        c = torch.full((m, n), -(2 ** 31), dtype=torch.int32, device=dev)
    else:
        c = torch.full((m, n), float("nan"), dtype=torch.float32, device=dev)
    gpu.m16_gemm(fmt, *ts, out=c)
    got = c.cpu().numpy().astype(np.float64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{fmt} {m}x{n}x{k}: {len(bad)} wrong elements, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")
    if fmt in m16.SCALED:  # and the 32×32 kernel on the same tensors, bit for bit
        other = gpu.mx_gemm(fmt, *ts)
        assert torch.equal(other.view(torch.int32), c.view(torch.int32))


# fewer than, equal to and more than the three stages in flight and the four ring slots, and a long K of 64 stages
K_STAGES = [1, 2, 3, 4, 5, 7, 64]
# one stage; workgroup counts = 0, 1 and 7 mod 8 (the XCD remap's three cases), then a single tile row of 11
GRIDS = [(512, 1024), (768, 768), (1280, 768), (256, 2816)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stages", K_STAGES)
def test_m16_gemm_exact_over_k(dev, fmt, stages):
    _exact_store(dev, fmt, 256, 256, stages * m16.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", GRIDS)
def test_m16_gemm_exact_over_grids(dev, fmt, m, n):
    _exact_store(dev, fmt, m, n, m16.STAGE[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_m16_gemm_exact_over_tiles_and_stages(dev, fmt):
    """2 × 3 tiles at 3 stages: operand addresses with a tile offset and ``kt > 0``."""
    _exact_store(dev, fmt, 512, 768, 3 * m16.STAGE[fmt])


# ------------------------------------------------------------------ fill and fused verify


def _model(fmt, m, n, k):
    """The operands the fills write, in the public layout on the host, and a ``product`` of such operands."""
    if fmt in m16.SCALED:
        code = m16.MX_CODE[fmt]
        va, vb = mx.probe_values(m, n, k)
        host = {"a": mx.encode(code, va), "bt": mx.encode(code, vb), "sa": mx.probe_scales(m, k),
                "sbt": mx.probe_scales(n, k)}
        expect = mx.probe_table(k)[np.arange(m)[:, None] % mx.ROWS, np.arange(n)[None, :] % mx.COLS]
        return host, expect, lambda h: mx.product(code, h["a"], h["bt"], h["sa"], h["sbt"])
    va, vb = ref.probe_operands(m, n, k)
    mul = (I8_MUL_A, I8_MUL_B) if fmt == "i8" else (1, 1)
    host = {"a": va * mul[0], "bt": vb * mul[1]}
    expect = (ref.probe_class_table(k) * mul[0] * mul[1])[np.arange(m)[:, None] % 5, np.arange(n)[None, :] % 7]
    return host, expect, lambda h: h["a"] @ h["bt"].T


def _filled(dev, fmt, m, n, k):
    a, bt, sa, sbt, table = _gpu().m16_fill(fmt, m, n, k, dev)
    return {"a": a, "bt": bt, "sa": sa, "sbt": sbt, "table": table}


def _verify(fmt, t):
    return _gpu().m16_verify(fmt, t["a"], t["bt"], t["sa"], t["sbt"], t["table"])


VERIFY_SHAPES = [(256, 256, s) for s in K_STAGES] + [(m, n, 1) for m, n in GRIDS] + [(512, 768, 3)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_m16_verify_clean(dev, fmt):
    for m, n, stages in VERIFY_SHAPES:
        k = stages * m16.STAGE[fmt]
        if fmt == "bf16" and k % 64:  # odh_probe_fill's own K granule is that of the 128² kernel; 32 divides all
            assert k % 32 == 0
        r = _verify(fmt, _filled(dev, fmt, m, n, k))
        assert r["errors"] == 0 and sum(r["err_xcd"]) == 0, (m, n, k, r)
        assert sum(r["xcd_blocks"]) == (m // 256) * (n // 256), (m, n, k, r)


def _host_to_dev(fmt, name, row):
    if name in ("sa", "sbt") or fmt in m16.SCALED:
        return torch.from_numpy(np.ascontiguousarray(row))
    return torch.from_numpy(row.astype(np.float32 if fmt != "i8" else np.int8)).to(TORCH_DTYPE[fmt])


def _sweep_rows(dev, fmt, name, changes):
    """One launch per ``(row, wrong host row)`` of operand ``name``: that row replaced on the GPU, the fused check,
    the row restored; the mismatch count and its per-XCD sum against the host product of the changed operands."""
    m, n = 256, 256
    k = 2 * m16.STAGE[fmt]
    host, expect, product = _model(fmt, m, n, k)
    assert np.array_equal(product(host), expect)  # the model agrees with itself: a clean run counts nothing
    t = _filled(dev, fmt, m, n, k)
    target = t[name]
    for x, (i, wrong_row) in enumerate(changes(host[name])):
        wrong = host[name].copy()
        wrong[i] = wrong_row
        clean_dev = target[i].clone()
        target[i].copy_(_host_to_dev(fmt, name, wrong[i]).view(target.dtype))
        r = _verify(fmt, t)
        target[i].copy_(clean_dev)
        bad = product(dict(host, **{name: wrong})) != expect
        want = int(bad.sum())
        assert 0 < want <= n and not np.delete(bad, i, axis=0).any(), (fmt, name, x)
        assert r["errors"] == want and sum(r["err_xcd"]) == want, (fmt, name, x, i, want, r)
        assert sum(r["xcd_blocks"]) == 1
    assert _verify(fmt, t)["errors"] == 0  # restored


@pytest.mark.parametrize("fmt", FORMATS)
def test_m16_verify_counts_a_changed_element_at_every_k_of_a_stage(dev, fmt):
    """``A[i][k]`` one value higher (i8: one multiple of 25 higher) at every k of the second stage, in a row that
    moves with k: the mismatches are the columns whose ``Bt[j][k]`` is not 0."""
    stage = m16.STAGE[fmt]

    def changes(clean):
        for j in range(stage):
            i, k = (37 * j + 5) % 256, stage + j
            if fmt in m16.SCALED:
                v = mx.probe_values(256, 1, 2 * stage)[0][i].copy()
                v[k] += 1
                yield i, mx.encode(m16.MX_CODE[fmt], v[None])[0]
            else:
                row = clean[i].copy()
                row[k] += I8_MUL_A if fmt == "i8" else 1
                yield i, row

    _sweep_rows(dev, fmt, "a", changes)


@pytest.mark.parametrize("fmt", m16.SCALED)
def test_m16_verify_counts_a_changed_scale_byte_in_every_block(dev, fmt):
    """``sA[i][b]`` one higher, which doubles that block of the row, for each of the row's eight blocks."""

    def changes(clean):
        assert clean.shape[1] == 8
        for b in range(8):
            i = (37 * b + 11) % 256
            row = clean[i].copy()
            row[b] += 1
            yield i, row

    _sweep_rows(dev, fmt, "sa", changes)


def test_m16_probe_runs_on_the_matrix_cores(dev):
    for fmt in FORMATS:
        r = _gpu().m16_probe(0, fmt, 512, 512, 384)
        assert set(r) == {"errors", "err_xcd", "xcd_blocks", "ms", "tflops"}
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == 4 and r["ms"] > 0
        _gpu().m16_probe(0, fmt)  # warm: the first launch of a kernel carries its code's first touch
        r = _gpu().m16_probe(0, fmt)
        print(f"m16_probe {fmt}: {r['ms']:.4f} ms, {r['tflops']:.1f} T(FL)OP/s")
        assert r["errors"] == 0 and sum(r["xcd_blocks"]) == 256
        assert r["tflops"] > 50, (fmt, r)  # the project's floor for "ran on the matrix cores"


# ------------------------------------------------------------------ entry points refuse


@pytest.mark.parametrize("fmt", FORMATS)
def test_m16_entry_points_check_before_launch(dev, fmt):
    gpu = _gpu()
    k = 2 * m16.STAGE[fmt]
    arrays, _ = _random_case(fmt, 256, 256, k)
    ts = _to_dev(dev, fmt, arrays)
    ta, tb, rest = ts[0], ts[1], ts[2:]
    other = torch.float32
    for fn in (gpu.m16_gemm, gpu.m16_verify):
        with pytest.raises(ValueError):
            fn("bf8", ta, tb, *rest)
        with pytest.raises(TypeError):
            fn(fmt, ta.to(other), tb, *rest)
        with pytest.raises(ValueError):
            fn(fmt, ta.t(), tb, *rest)  # not contiguous
        with pytest.raises(ValueError):
            fn(fmt, ta[:128].contiguous(), tb, *rest)  # M = 128
        with pytest.raises(ValueError):
            fn(fmt, ta, tb[:, :tb.shape[1] // 2].contiguous(), *rest)  # K of A and of Bt differ
        with pytest.raises(ValueError):
            fn(fmt, ta.cpu(), tb, *rest)  # not on the same device
        if fmt in m16.SCALED:
            with pytest.raises(ValueError):
                fn(fmt, ta, tb)  # no scales
            with pytest.raises(ValueError):
                fn(fmt, ta, tb, rest[0][:, :1].contiguous(), rest[1])
        else:
            s = torch.zeros((256, k // 32), dtype=torch.uint8, device=dev)
            with pytest.raises(ValueError):
                fn(fmt, ta, tb, s, s)  # scales with a format that takes none
    with pytest.raises(ValueError):
        gpu.m16_verify(fmt, ta, tb, *rest, table=None if fmt in m16.SCALED else torch.zeros(gpu.MX_TABLE, device=dev))
    good = torch.int32 if fmt == "i8" else torch.float32
    for out in (torch.empty((256, 256), dtype=torch.int32 if good == torch.float32 else torch.float32, device=dev),
                torch.empty((256, 128), dtype=good, device=dev), torch.empty((256, 256), dtype=good)):
        with pytest.raises(ValueError):
            gpu.m16_gemm(fmt, ta, tb, *rest, out=out)
    regs = torch.zeros((64, 8), dtype=torch.int32, device=dev)
    sc = torch.zeros((64,), dtype=torch.int32, device=dev)
    s2 = (sc, sc) if fmt in m16.SCALED else ()
    for bad in (lambda: gpu.m16_one(fmt, regs[:, :4].contiguous(), regs, *s2), lambda: gpu.m16_one(fmt, regs, regs.cpu(), *s2),
                lambda: gpu.m16_one(fmt, regs, regs, *s2, opsel_a=4), lambda: gpu.m16_one(fmt, regs, regs, *s2, opsel_b=-1),
                lambda: gpu.m16_one(fmt, regs, regs, *(() if s2 else (sc, sc)))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        gpu.m16_one(fmt, regs.float(), regs, *s2)


def test_m16_c_abi_refuses_before_launch(dev):
    """The library's own checks, below the Python ones: ``hipErrorInvalidValue`` and no launch."""
    gpu = _gpu()
    lib = gpu.load_library()
    invalid = 1  # hipErrorInvalidValue
    a = torch.zeros((256, 128), dtype=torch.uint8, device=dev)
    bt = torch.zeros((256, 128), dtype=torch.uint8, device=dev)
    sc = torch.zeros((256, 4), dtype=torch.uint8, device=dev)
    tab = torch.zeros(gpu.MX_TABLE, dtype=torch.float32, device=dev)
    c = torch.zeros((256, 256), dtype=torch.int32, device=dev)
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pa, pb, ps, pt, pc, pk = (x.data_ptr() for x in (a, bt, sc, tab, c, counters))
    bf16, f16, i8, fp8, fp4 = (gpu.M16_FORMATS[f] for f in FORMATS)
    for args in ((5, pa, pb, None, None, 256, 256, 64), (-1, pa, pb, None, None, 256, 256, 64),  # unknown formats
                 (i8, pa, pb, None, None, 128, 256, 128), (i8, pa, pb, None, None, 256, 384, 128),
                 (i8, pa, pb, None, None, 256, 256, 32), (bf16, pa, pb, None, None, 256, 256, 16),
                 (f16, pa, pb, None, None, 256, 256, 0), (fp8, pa, pb, ps, ps, 256, 256, 64),
                 (fp4, pa, pb, ps, ps, 256, 256, 192),
                 (i8, None, pb, None, None, 256, 256, 128), (i8, pa, None, None, None, 256, 256, 128),
                 (i8, pa + 8, pb, None, None, 256, 256, 64), (fp8, pa, pb + 4, ps, ps, 256, 256, 128),  # alignment
                 (fp8, pa, pb, ps + 2, ps, 256, 256, 128), (fp4, pa, pb, ps, ps + 1, 256, 256, 128),
                 (i8, pa, pb, ps, None, 256, 256, 128), (bf16, pa, pb, None, ps, 256, 256, 64),  # scales, dense format
                 (fp8, pa, pb, None, ps, 256, 256, 128), (fp4, pa, pb, ps, None, 256, 256, 128)):  # none, scaled format
        fmt, xa, xb, xs, xt, m, n, k = args
        assert lib.odh_m16_gemm(fmt, xa, xb, xs, xt, pc, m, n, k, s) == invalid, args
        table = pt if fmt in (fp8, fp4) else None
        assert lib.odh_m16_probe_gemm_verify(fmt, xa, xb, xs, xt, table, m, n, k, None, pk, s) == invalid, args
    assert lib.odh_m16_gemm(i8, pa, pb, None, None, None, 256, 256, 128, s) == invalid
    assert lib.odh_m16_probe_gemm_verify(i8, pa, pb, None, None, None, 256, 256, 128, None, None, s) == invalid
    assert lib.odh_m16_probe_gemm_verify(i8, pa, pb, None, None, pt, 256, 256, 128, None, pk, s) == invalid
    assert lib.odh_m16_probe_gemm_verify(fp8, pa, pb, ps, ps, None, 256, 256, 128, None, pk, s) == invalid
    for args in ((5, pa, pb, ps, ps, 0, 0), (fp8, pa, pb, ps, ps, 4, 0), (fp8, pa, pb, ps, ps, 0, -1),
                 (fp4, pa + 4, pb, ps, ps, 0, 0), (fp4, pa, pb, None, ps, 0, 0), (bf16, pa, pb, ps, ps, 0, 0),
                 (bf16, pa, pb, None, None, 0, 4), (i8, None, pb, None, None, 0, 0)):
        fmt, xa, xb, xs, xt, oa, ob = args
        assert lib.odh_m16_one(fmt, xa, xb, xs, xt, oa, ob, pc, s) == invalid, args
    assert lib.odh_m16_one(fp8, pa, pb, ps, ps, 0, 0, None, s) == invalid
    torch.cuda.synchronize(dev)
    assert int(c.abs().sum()) == 0 and int(counters.abs().sum()) == 0 and int(a.sum()) == 0 and int(tab.abs().sum()) == 0


# ------------------------------------------------------------------ the program

ALL = "bf16,f16,i8,fp8,fp4"
KEYS_WITHOUT = ["ok", "devices", "shape", "hbm_mib", "results", "links", "setup_ms", "timings_ms"]


def test_mfma16_program_passes_with_every_format():
    rc, res, r = _run_probe("--mfma16", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["mfma16"]) == ["ok", "errors", "ms", "bad"]
    f = res["mfma16"]
    assert f["ok"] is True and f["errors"] == 0 and f["bad"] == "" and f["ms"] > 0
    assert list(res) == KEYS_WITHOUT[:6] + ["mfma16"] + KEYS_WITHOUT[6:]
    t = list(res["timings_ms"])
    assert t.index("rccl") < t.index("mfma16") < t.index("total") and res["timings_ms"]["mfma16"] > 0
    print("verdict bytes:", len(r.stdout.strip().splitlines()[-1]), "mfma16:", f, res["timings_ms"])
    # a subset, in another order
    rc, res, r = _run_probe("--mfma16", "fp4,bf16,i8")
    assert rc == 0 and res["mfma16"]["ok"] is True and res["mfma16"]["bad"] == "", r.stdout


def test_mfma16_program_after_every_other_step_under_the_message_limit():
    rc, res, r = _run_probe("--mx", "fp8,fp4,bf8,fp6,bf6", "--dtypes", "f16,i8", "--fp", "f32,f64", "--sparse",
                            "bf16,f16,i8,fp8,bf8", "--cvt", "fp8,bf8,fp4,fp6,bf6,bf16", "--lds",
                            "mem,tr16,tr8,tr4,tr6,xlane", "--mfma16", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    keys = list(res)
    assert keys.index("cvt") < keys.index("lds") < keys.index("mfma16")
    assert keys[-3:] == ["mfma16", "setup_ms", "timings_ms"]
    assert list(res["timings_ms"])[-3:] == ["lds", "mfma16", "total"]
    assert res["mfma16"]["ok"] is True and res["mx"]["fp8"]["ok"] is True
    line = r.stdout.strip().splitlines()[-1]
    print("verdict bytes:", len(line))
    assert len(line) < 4096
    # the scales and the table serve --mfma16 alone too, before and after a step that does not use them
    rc, res, r = _run_probe("--dtypes", "f16,i8", "--mfma16", "fp8,fp4")
    assert rc == 0 and res["mfma16"]["ok"] is True, r.stdout


def test_mfma16_program_without_the_step_is_what_it_was():
    rc, res, r = _run_probe()
    assert rc == 0 and res["ok"], r.stdout
    assert list(res) == KEYS_WITHOUT and "mfma16" not in res and "mfma16" not in res["timings_ms"]
    assert list(res["timings_ms"]) == ["exec", "hip_init", "alloc_fill", "alloc", "code_load", "fill", "probe", "xgmi",
                                       "rccl", "total"]
    rc, res, r = _run_probe("--lds", "xlane")
    assert rc == 0 and list(res) == KEYS_WITHOUT[:6] + ["lds"] + KEYS_WITHOUT[6:]


def test_mfma16_program_fails_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    # A[0][0] becomes another value: row 0 is wrong exactly where Bt[j][0] = ((11 j) mod 7) - 3 is non-zero
    _, vb = ref.probe_operands(1, 4096, 1)
    want = int((vb[:, 0] != 0).sum())
    assert 0 < want < 4096
    for asked in (ALL, "fp8,f16"):
        rc, res, r = _run_probe("--mfma16", asked, "--inject-fault", "mfma16")
        assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
        f = res["mfma16"]
        assert res["ok"] is False and f["ok"] is False and f["bad"] == asked, f
        assert f["errors"] == want * len(asked.split(",")), f
        first = asked.split(",")[0]
        assert "GPU 0" in res["error"] and f"mfma16 {first}" in res["error"] and "16x16 GEMM mismatches" in res["error"]
        d = res["results"][0]
        assert d["ok"] is True and d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
        assert len(r.stdout.strip().splitlines()[-1]) < 4096
    print(json.dumps(res["mfma16"]))
