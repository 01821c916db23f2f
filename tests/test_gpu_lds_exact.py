"""The LDS step of the start-up probe and the transposer of packed codes, on an MI355X.

* one transposing LDS read (``lds_tr_read``) and one lane exchange (``lds_xlane``) against the host model
  (``lds_reference.py``) bit for bit: blocks at every aligned offset of a bank row, three pitches, the four groups
  of lanes on different blocks, misaligned addresses; every op and selector;
* the fused checks: clean on a healthy device, and with one table byte wrong exactly the model's count;
* ``transpose_codes`` bit for bit in every format, its refusals, and ``mx_transpose`` through ``mx_gemm``;
* ``odh-gpu-probe --lds``.

The tests corrupt data only: a wrong table byte is wrong data, and every address handed to ``lds_tr_read`` is
checked against the image's size before anything is launched.
"""

import numpy as np
import pytest

import lds_reference as lr
from probe_gpu import _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TR = ["tr16", "tr8", "tr4", "tr6"]
CHECKS = list(lr.NAMES)
ALL = ",".join(CHECKS)

# ------------------------------------------------------------------ the maps


@pytest.mark.parametrize("name", TR)
def test_transposing_read_is_the_models(dev, name):
    """A seeded random image; per launch the four groups of lanes read four different blocks of it.  The blocks'
    base visits every aligned offset of a 256-byte bank row, at three row pitches, one of them no power of two."""
    gpu = _gpu()
    check = lr.NAMES[name]
    _, rows, align, slot, width = lr.TR[check]
    rng = np.random.default_rng(40 + check)
    host = rng.integers(0, 256, 16384, dtype=np.uint8)
    image = torch.from_numpy(host).to(dev)
    launches = 0
    for pitch in (2 * slot, 2 * slot + align, 8 * slot):
        assert pitch % align == 0
        for at, base in enumerate(range(0, 256, align)):
            # group g: the block g row blocks down and (g + at) mod 2 column blocks along
            addr = [base + g * rows * pitch + ((g + at) % 2) * slot + lr.tr_lane_offset(check, i, pitch)
                    for g in range(4) for i in range(16)]
            assert len({a for a in addr}) == 64 and max(addr) + width <= host.size
            got = gpu.lds_tr_read(name, image, addr).cpu().numpy()
            want = lr.tr_read(check, host, addr)
            assert np.array_equal(got, want), (name, pitch, base, np.argwhere(got != want)[:4].tolist())
            launches += 1
    assert launches == 3 * 256 // align
    assert any(p & (p - 1) for p in (2 * slot, 2 * slot + align, 8 * slot))


@pytest.mark.parametrize("name", TR)
def test_transposing_read_refuses_bad_addresses_and_drops_low_address_bits(dev, name):
    gpu = _gpu()
    check = lr.NAMES[name]
    _, _, align, _, width = lr.TR[check]
    host = np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8)
    image = torch.from_numpy(host).to(dev)
    good = [64 * lane for lane in range(64)]
    lib = gpu.load_library()
    out = torch.zeros((64, width), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    import ctypes

    for lane, bad in ((0, 4096), (63, 4096 - width + align), (5, 64 * 5 + align // 2), (17, 64 * 17 + 4), (40, 2 ** 31)):
        addr = list(good)
        addr[lane] = bad
        with pytest.raises(ValueError):
            gpu.lds_tr_read(name, image, addr)
        arr = (ctypes.c_uint32 * 64)(*addr)
        rc = lib.odh_lds_tr_read(check, image.data_ptr(), 4096, ctypes.cast(arr, ctypes.c_void_p), out.data_ptr(), st)
        assert rc == 1, (lane, bad)  # hipErrorInvalidValue, before anything is launched
    torch.cuda.synchronize(dev)
    assert not out.any()
    for bad in (image[:4094], image.to(torch.int8), image.cpu(), image.reshape(64, 64)):
        with pytest.raises(ValueError):
            gpu.lds_tr_read(name, bad, good)
    with pytest.raises(ValueError):
        gpu.lds_tr_read(name, image, good[:63])
    with pytest.raises(ValueError):
        gpu.lds_tr_read("mem", image, good)
    # what the instruction does with an address that is not aligned (measuring mode): it reads from the aligned
    # address below, with no error
    for off in (1, 2, 4, align - 2, align + 4):
        addr = [a + off for a in good]
        got = gpu.lds_tr_read(name, image, addr, raw=True).cpu().numpy()
        assert np.array_equal(got, lr.tr_read(check, host, addr)), off
        assert np.array_equal(got, lr.tr_read(check, host, [a + off // align * align for a in good])), off


@pytest.mark.parametrize("op", list(lr.OPS))
def test_lane_exchange_is_the_models(dev, op):
    gpu = _gpu()
    n = 128 if op.endswith("_swap") else 64
    rng = np.random.default_rng(60 + lr.OPS[op])
    host = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    assert len(set(host.tolist())) == n
    values = torch.from_numpy(host).to(dev)
    outs = torch.stack([gpu.lds_xlane(op, arg, values) for arg in range(lr.ARGS[op])]).cpu().numpy()
    for arg in range(lr.ARGS[op]):
        want = host[lr.xl_sources(op, arg)]
        assert np.array_equal(outs[arg], want), (op, arg, outs[arg].tolist(), want.tolist())
    assert np.array_equal(values.cpu().numpy(), host)
    with pytest.raises(ValueError):
        gpu.lds_xlane(op, lr.ARGS[op], values)
    with pytest.raises(ValueError):
        gpu.lds_xlane(op, 0, values[:n - 1])


# ------------------------------------------------------------------ the fused checks


@pytest.mark.parametrize("name", CHECKS)
def test_fused_check_clean_and_with_one_table_byte_wrong(dev, name):
    gpu = _gpu()
    check = lr.NAMES[name]
    table = torch.full((gpu.ODH_LDS_TABLE,), 0xEE, dtype=torch.uint8, device=dev)
    gpu.lds_fill(name, table)
    assert np.array_equal(table.cpu().numpy(), lr.table(check))
    r = gpu.lds_verify(name, table)
    assert set(r) == {"ok", "errors", "blocks", "err_xcd", "xcd_blocks", "ms", "cus"}
    assert r["ok"] is True and r["errors"] == 0 and sum(r["err_xcd"]) == 0, r
    assert r["blocks"] == sum(r["xcd_blocks"]) == gpu.ODH_LDS_BLOCKS == 256 and all(b > 0 for b in r["xcd_blocks"]), r
    assert r["ms"] > 0 and 0 < r["cus"] <= 256, r
    print(name, "cus:", r["cus"], "ms:", r["ms"])
    # the first and the last byte, and one of every other position in a dword; a flipped bit 0 is a change that
    # no element's fold misses, and 0x5A (tr4 and tr6: 0x53, the nibbles change differently) another
    for at, delta in ((0, 1), (1, 0x53 if check in (lr.TR4, lr.TR6) else 0x5A), (514, 0x80), (771, 1), (1023, 1)):
        assert lr.fold_changes(check, delta)
        table[at] ^= delta
        bad = gpu.lds_verify(name, table)
        table[at] ^= delta
        want = gpu.lds_fault_count(name, at)
        assert want == lr.fault_count(check, at) > 0
        assert bad["errors"] == want and bad["ok"] is False, (name, at, bad, want)
        assert sum(bad["err_xcd"]) == want and bad["blocks"] == 256, (at, bad)
        # every workgroup meets the same cases
        assert bad["err_xcd"] == [want // 256 * b for b in bad["xcd_blocks"]], (at, bad)
    assert np.array_equal(table.cpu().numpy(), lr.table(check))
    again = gpu.lds_probe(0, name)
    assert again["ok"] and again["errors"] == 0 and again["blocks"] == 256


def test_fused_check_entry_points_check_before_launch(dev):
    gpu = _gpu()
    table = torch.zeros(gpu.ODH_LDS_TABLE, dtype=torch.uint8, device=dev)
    for fn in (gpu.lds_fill, gpu.lds_verify):
        for bad_t in (table[:1023], table.to(torch.int8), table.cpu(), torch.zeros(1028, dtype=torch.uint8, device=dev)[1:1025]):
            with pytest.raises(ValueError):
                fn("mem", bad_t)
        for bad in ("tr32", 6, -1):
            with pytest.raises(ValueError):
                fn(bad, table)
    lib = gpu.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    counters = torch.zeros(gpu.ODH_NCOUNT + gpu.ODH_LDS_CU_WORDS, dtype=torch.int32, device=dev)
    assert lib.odh_lds_fill(6, table.data_ptr(), st) == 1 and lib.odh_lds_fill(0, table.data_ptr() + 2, st) == 1
    assert lib.odh_lds_probe_verify(6, table.data_ptr(), counters.data_ptr(), st) == 1
    assert lib.odh_lds_probe_verify(0, None, counters.data_ptr(), st) == 1
    assert lib.odh_lds_probe_verify(0, table.data_ptr(), None, st) == 1
    torch.cuda.synchronize(dev)
    assert not table.any() and not counters.any()


# ------------------------------------------------------------------ the transposer

SHAPES = [(128, 128), (256, 384), (384, 128)]


def _codes(fmt, rows, cols, seed):
    rng = np.random.default_rng(seed)
    bits = lr.FORMAT_BITS[fmt]
    if bits == 16:
        return rng.integers(0, 1 << 16, (rows, cols), dtype=np.uint16)
    return rng.integers(0, 256, (rows, cols * bits // 8), dtype=np.uint8)


def _to_dev(fmt, host, dev):
    t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
    return t.view({"bf16": torch.bfloat16, "f16": torch.float16}[fmt]) if host.dtype == np.uint16 else t


def _to_host(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.element_size() == 2 else t.cpu().numpy()


@pytest.mark.parametrize("fmt", list(lr.FORMAT_BITS))
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_transpose_codes_is_the_models(dev, fmt, rows, cols):
    gpu = _gpu()
    host = _codes(fmt, rows, cols, 100 + rows + cols)
    x = _to_dev(fmt, host, dev)
    t = gpu.transpose_codes(fmt, x)
    want = lr.transpose_codes(fmt, host)
    got = _to_host(t)
    assert got.shape == want.shape and t.dtype == x.dtype
    assert np.array_equal(got, want), (fmt, np.argwhere(got != want)[:6].tolist())
    assert np.array_equal(_to_host(x), host)  # the source is left alone
    assert np.array_equal(_to_host(gpu.transpose_codes(fmt, t)), host)


def test_transpose_codes_refuses_before_launch(dev):
    gpu = _gpu()
    x = torch.zeros((128, 256), dtype=torch.uint8, device=dev)
    for fmt, bad in (("fp8", x[:, :64].contiguous()), ("fp8", x[:64]), ("fp4", x[:, :32].contiguous()),
                     ("fp6", x[:, :48].contiguous()), ("fp6", x[:, :100].contiguous()),  # 64 columns; no whole elements
                     ("fp8", x[:, :128]), ("fp8", x.t()),  # not contiguous
                     ("fp8", x.to(torch.int8)), ("bf16", x), ("f16", x.view(torch.bfloat16)), ("fp8", x.cpu()),
                     ("fp8", x.reshape(2, 64, 256)), ("fp5", x), ("fp8", x[:, :192].contiguous()[:, :0])):
        with pytest.raises(ValueError):
            gpu.transpose_codes(fmt, bad)
    flat = torch.zeros(128 * 128 + 16, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="aligned"):
        gpu.transpose_codes("fp8", flat[4:4 + 128 * 128].reshape(128, 128))  # contiguous, 4 bytes off
    lib = gpu.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    out = torch.zeros((128, 128), dtype=torch.uint8, device=dev)
    px, po = flat.data_ptr(), out.data_ptr()
    for args in ((4, px, po, 128, 128), (1, px, po, 128, 64), (1, px, po, 64, 128), (1, px, po, 0, 128),
                 (1, None, po, 128, 128), (1, px, None, 128, 128), (1, px + 4, po, 128, 128), (1, px, po + 4, 128, 128),
                 (1, px, px, 128, 128)):
        assert lib.odh_transpose_codes(*args, st) == 1, args
    torch.cuda.synchronize(dev)
    assert not out.any()


@pytest.mark.parametrize("fmt", ["fp8", "fp4", "fp6"])
def test_mx_transpose_feeds_the_matrix_cores(dev, fmt):
    """B held as ``[K][N]`` codes with ``[K/32][N]`` scales, random: ``mx_gemm`` with ``mx_transpose``'s output is
    ``mx_gemm`` with the operands transposed on the host, bit for bit."""
    gpu = _gpu()
    rng = np.random.default_rng(200 + lr.FORMAT_BITS[fmt])
    m, n, k = 256, 256, 128
    bits = lr.FORMAT_BITS[fmt]
    b = rng.integers(0, 256, (k, n * bits // 8), dtype=np.uint8)
    sb = rng.integers(120, 135, (k // 32, n), dtype=np.uint8)
    a = rng.integers(0, 256, (m, k * bits // 8), dtype=np.uint8)
    sa = rng.integers(120, 135, (m, k // 32), dtype=np.uint8)
    bt_host, sbt_host = lr.transpose_codes(fmt, b), np.ascontiguousarray(sb.T)
    bt, sbt = gpu.mx_transpose(fmt, torch.from_numpy(b).to(dev), torch.from_numpy(sb).to(dev))
    assert np.array_equal(bt.cpu().numpy(), bt_host) and np.array_equal(sbt.cpu().numpy(), sbt_host)
    assert bt.is_contiguous() and sbt.is_contiguous() and tuple(sbt.shape) == (n, k // 32)
    da, dsa = torch.from_numpy(a).to(dev), torch.from_numpy(sa).to(dev)
    got = gpu.mx_gemm(fmt, da, bt, dsa, sbt)
    want = gpu.mx_gemm(fmt, da, torch.from_numpy(bt_host).to(dev), dsa, torch.from_numpy(sbt_host).to(dev))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert got.abs().nan_to_num().max() > 0


# ------------------------------------------------------------------ the program

KEYS_WITHOUT = ["ok", "devices", "shape", "hbm_mib", "results", "links", "setup_ms", "timings_ms"]


def test_lds_program_passes_with_every_check():
    rc, res, r = _run_probe("--lds", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    assert res["ok"] and list(res["lds"]) == ["ok", "errors", "ms", "bad"]
    assert res["lds"]["ok"] is True and res["lds"]["errors"] == 0 and res["lds"]["bad"] == "" and res["lds"]["ms"] > 0
    assert list(res) == KEYS_WITHOUT[:6] + ["lds"] + KEYS_WITHOUT[6:]
    t = list(res["timings_ms"])
    assert t.index("rccl") < t.index("lds") < t.index("total") and res["timings_ms"]["lds"] > 0
    print("verdict bytes:", len(r.stdout.strip().splitlines()[-1]), "lds:", res["lds"], res["timings_ms"])
    # a subset, in another order
    rc, res, r = _run_probe("--lds", "xlane,mem")
    assert rc == 0 and res["lds"]["ok"] is True and res["lds"]["bad"] == "", r.stdout


def test_lds_program_after_every_other_step_under_the_message_limit():
    rc, res, r = _run_probe("--mx", "fp8,fp4,bf8,fp6,bf6", "--dtypes", "f16,i8", "--fp", "f32,f64", "--sparse",
                            "bf16,f16,i8,fp8,bf8", "--cvt", "fp8,bf8,fp4,fp6,bf6,bf16", "--lds", ALL)
    assert rc == 0, (r.stdout, r.stderr)
    keys = list(res)
    assert keys.index("sparse") < keys.index("cvt") < keys.index("lds")
    assert keys[-3:] == ["lds", "setup_ms", "timings_ms"]
    assert list(res["timings_ms"])[-3:] == ["cvt", "lds", "total"]
    line = r.stdout.strip().splitlines()[-1]
    print("verdict bytes:", len(line))
    assert len(line) < 4096


def test_lds_program_without_the_step_is_what_it_was():
    rc, res, r = _run_probe()
    assert rc == 0 and res["ok"], r.stdout
    assert list(res) == KEYS_WITHOUT and "lds" not in res and "lds" not in res["timings_ms"]
    assert list(res["timings_ms"]) == ["exec", "hip_init", "alloc_fill", "alloc", "code_load", "fill", "probe", "xgmi",
                                       "rccl", "total"]


def test_lds_program_fails_on_injected_fault():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--lds", ALL, "--inject-fault", "lds")
    assert rc == probe_main.CHECK_FAILED, (r.stdout, r.stderr)
    assert res["ok"] is False and res["lds"]["ok"] is False
    assert res["lds"]["bad"] == ALL  # every check asked for met the wrong key
    assert res["lds"]["errors"] == sum(lr.fault_count(c, 5) for c in lr.NAMES.values())
    assert "GPU 0" in res["error"] and "lds mem" in res["error"] and "LDS mismatches" in res["error"], res["error"]
    assert "on XCD 0,1,2,3,4,5,6,7" in res["error"] and "256/256" in res["error"], res["error"]
    d = res["results"][0]
    assert d["ok"] is True and d["gemm_errors"] == 0 and d["hbm_errors"] == 0, d
    assert len(r.stdout.strip().splitlines()[-1]) < 4096
    # a subset fails in the checks asked for only
    rc, res, r = _run_probe("--lds", "tr6,xlane", "--inject-fault", "lds")
    assert rc == probe_main.CHECK_FAILED and res["lds"]["bad"] == "tr6,xlane", r.stdout
