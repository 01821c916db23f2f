"""The vector-memory step on the GPU: ``vmem_access`` one access per lane against NumPy slicing, the four fused
checks of ``--vmem`` clean and with one table byte changed, and the program."""

import numpy as np
import pytest

from probe_gpu import _gpu, _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

gpu = _gpu()
FAULT_BYTES = (5, 770)  # tests/test_probe_vmem.py holds their counts above 0
IMM, SOFF, GUARD = gpu.ODH_VM_ACCESS_IMM, 256, gpu.ODH_VM_GUARD


def _image():
    img = np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8)
    img[0::7], img[1::7], img[2::7] = 0x7F, 0x80, 0xFF  # both sign-bit states under every extending load
    return img


def _register(op, piece):
    """The 16 bytes of a lane's register(s) after a load of ``piece``."""
    out = np.zeros(16, dtype=np.uint8)
    out[:len(piece)] = piece
    if op in ("ld_i8", "ld_i16") and piece[-1] & 0x80:
        out[len(piece):4] = 0xFF
    if op == "ld_d16_hi":  # the other half of either d16 load reads 0 whatever it held: the MI355X runs with SRAM ECC
        out[0:2], out[2:4] = 0, piece
    return out


def _model(op, img, off, data, nr, soff, imm, lds_base):
    """(out [64][16], image after) of one access per lane: ``img[off : off + w]`` as the op says."""
    _, kind, w = gpu.VMEM_OPS[op]
    after, out = img.copy(), np.zeros((64, 16), dtype=np.uint8)
    lds = np.full(65536 + 16, 0xEE, dtype=np.uint8)
    stride = 16 if w == 12 else w  # a 12-byte LDS-DMA lane has a 16-byte slot
    buffer = kind in ("bufld", "bufst", "dmabuf")
    for lane, o in enumerate(off):
        at = o + imm + (soff if buffer else 0)
        # the range check counts all three offsets and is made per dword: of an access that the range cuts, the
        # dwords in range arrive (or land) and the others are zeros (or dropped)
        n = w if not buffer else 0 if at + min(w, 4) > nr else min(w, (nr - at) // 4 * 4) if w > 4 else w
        piece = np.concatenate([img[at:at + n], np.zeros(w - n, dtype=np.uint8)])
        if kind in ("ld", "bufld"):
            out[lane] = _register(op, piece) if n else 0
        elif kind in ("st", "bufst"):
            after[at:at + n] = (data[lane][2:] if op.endswith("d16_hi") else data[lane])[:n]
        else:
            place = lds_base + imm + lane * stride
            lds[place:place + w] = piece
    if kind in ("dma", "dmabuf"):
        for lane in range(64):
            out[lane] = lds[lds_base + imm + lane * stride:][:16]
    return out, after


def _cases(op):
    """(lane offsets, num_records, soffset, imm, lds_base) of an op: contiguous, reversed and one address, 12-byte
    accesses across a 64- and a 128-byte line, every asked-for range of a buffer, two M0 bases."""
    _, kind, w = gpu.VMEM_OPS[op]
    lanes = np.arange(64)
    sets = [lanes * w, lanes[::-1] * w, np.full(64, 5 * 16)]
    if w == 12:
        sets.append(np.where(lanes % 2, 116, 52))
    if kind in ("ld", "st"):
        return [(s, 0, 0, 0, 0) for s in sets]
    if kind == "dma":
        return [(s, 0, 0, imm, base) for s in sets for imm, base in ((0, 0), (IMM, 4112))]
    ranges = [0, w, 63 * w, 64 * w, SOFF + IMM + w, SOFF + IMM + 63 * w]  # the last two end it mid-wave whatever w
    if kind == "dmabuf":
        return [(sets[0], nr, SOFF, IMM, base) for nr in ranges for base in (0, 4112)]
    return [(s, nr, SOFF, IMM, 0) for s in sets for nr in ranges]


@pytest.mark.parametrize("op", list(gpu.VMEM_OPS))
def test_one_access_per_lane_is_the_numpy_slice(dev, op):
    img = _image()
    image = torch.from_numpy(img).to(dev)
    rng = np.random.default_rng(11)
    for case, (off, nr, soff, imm, base) in enumerate(_cases(op)):
        data = rng.integers(0, 256, (64, 16), dtype=np.uint8)
        if len(set(off.tolist())) < 64:
            data[:] = data[0]  # lanes that store to one address store one value
        out, buf = gpu.vmem_access(op, image, off, torch.from_numpy(data).to(dev), nr, soff, imm, base)
        want_out, want_img = _model(op, img, off, data, nr, soff, imm, base)
        buf = buf.cpu().numpy()
        what = f"{op} case {case}: nr={nr} soff={soff} imm={imm} lds={base}"
        assert np.array_equal(out.cpu().numpy(), want_out), what
        assert np.array_equal(buf[GUARD:GUARD + img.size], want_img), what
        assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + img.size:] == 0xA5).all(), what + ": guard zone written"


def test_access_refuses_before_launch(dev):
    image = torch.zeros(4096, dtype=torch.uint8, device=dev)
    lanes = np.arange(64)
    for op, off, kw in [("ld_b128", lanes * 16 + 4096 - 63 * 16, {}), ("ld_b32", lanes * 4 + 2, {}),
                        ("st_b16", lanes * 2 + 1, {}), ("ld_u8", lanes, {"imm": IMM}),
                        ("buf_st_b128", lanes * 16, {"num_records": 64, "soffset": 4096 + GUARD - 1008}),
                        ("buf_ld_b32", lanes * 4, {"num_records": 4096 + GUARD + 4}),
                        ("dma_b128", lanes * 16, {"lds_base": 65536 - 1008})]:
        with pytest.raises(ValueError):
            gpu.vmem_access(op, image, off, **kw)
    lib, buf = gpu.load_library(), torch.zeros(2 * GUARD + 65536, dtype=torch.uint8, device=dev)
    data = torch.zeros((64, 16), dtype=torch.uint8, device=dev)
    off = (gpu.ctypes.c_uint32 * 64)(*[4096 - 8] * 64)
    assert lib.odh_vmem_access(gpu.VMEM_OPS["st_b128"][0], buf.data_ptr(), 4096, off, data.data_ptr(), 0, 0, 0, 0,
                               data.data_ptr(), 0) != 0
    assert lib.odh_vmem_access(gpu.ODH_VM_OPS, buf.data_ptr(), 4096, off, data.data_ptr(), 0, 0, 0, 0, data.data_ptr(), 0) != 0
    torch.cuda.synchronize()
    assert not buf.any()


@pytest.fixture(scope="module")
def arena(dev):
    return torch.empty(gpu.ODH_VM_BLOCKS * gpu.ODH_VM_SLAB, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("check", list(gpu.VMEM_CHECKS))
def test_fused_check_clean_and_with_one_table_byte_changed(dev, arena, check):
    table = torch.empty(gpu.ODH_VM_TABLE, dtype=torch.uint8, device=dev)
    gpu.vmem_fill(check, table)
    r = gpu.vmem_verify(check, table, arena)
    print(check, r)
    assert r["ok"] and r["errors"] == 0 and r["blocks"] == gpu.ODH_VM_BLOCKS, r
    assert r["xcd_blocks"] == [gpu.ODH_VM_BLOCKS // gpu.N_XCD] * gpu.N_XCD and r["cus"] == gpu.ODH_VM_BLOCKS, r
    for byte, flip in zip(FAULT_BYTES, (0x01, 0x80)):
        want = gpu.vmem_fault_count(check, byte)
        assert want > 0
        table[byte] ^= flip
        r = gpu.vmem_verify(check, table, arena)
        table[byte] ^= flip
        assert r["errors"] == want and sum(r["err_xcd"]) == want and r["blocks"] == gpu.ODH_VM_BLOCKS, (byte, want, r)


def test_program_runs_the_step_and_names_the_faulted_check():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--vmem", "cache,sub,buf,dma")
    assert rc == 0 and res["ok"], (r.stdout, r.stderr)
    assert res["vmem"]["ok"] is True and res["vmem"]["errors"] == 0 and res["vmem"]["bad"] == "" and res["vmem"]["ms"] > 0
    assert list(res)[-3:] == ["vmem", "setup_ms", "timings_ms"] and list(res["timings_ms"])[-2:] == ["vmem", "total"]
    print("vmem:", res["vmem"], res["timings_ms"])
    rc, res, r = _run_probe("--vmem", "sub,dma,cache", "--inject-fault", "vmem")
    assert rc == probe_main.CHECK_FAILED and res["ok"] is False, (r.stdout, r.stderr)
    assert res["vmem"]["bad"] == "sub" and res["vmem"]["errors"] == gpu.vmem_fault_count("sub", 5), res["vmem"]
    assert "vmem sub" in res["error"] and res["results"][0]["ok"] is True
    rc, res, r = _run_probe("--vmem", "cache", "--hbm-mib", "8")
    assert rc == probe_main.USAGE and r.stdout == ""


def test_program_carves_every_region_and_any_subset():
    """All eight steps with every format share one device block and one counters region; then regions missing
    between present ones, with the MX tables there for ``--mfma16 fp4`` alone."""
    every = {"mx": "fp8,fp4,bf8,fp6,bf6", "dtypes": "f16,i8", "fp": "f32,f64", "sparse": "bf16,f16,i8,fp8,bf8",
             "cvt": "fp8,bf8,fp4,fp6,bf6,bf16", "lds": "mem,tr16,tr8,tr4,tr6,xlane", "mfma16": "bf16,f16,i8,fp8,fp4",
             "vmem": "cache,sub,buf,dma"}
    rc, res, r = _run_probe(*[a for word, formats in every.items() for a in ("--" + word, formats)])
    assert rc == 0 and res["ok"], (r.stdout, r.stderr)
    assert list(res)[-3:] == ["vmem", "setup_ms", "timings_ms"]
    assert [k for k in res if k in every] == list(every)
    for word, formats in every.items():
        entries = [res[word]] if "bad" in res[word] else [res[word][f] for f in formats.split(",")]
        assert all(e["ok"] is True and e["errors"] == 0 for e in entries), (word, res[word])
    line = r.stdout.strip().splitlines()[-1]
    assert len(line.encode()) < 4096
    print("every step:", len(line), "bytes", res["timings_ms"])
    rc, res, r = _run_probe("--sparse", "i8", "--lds", "mem", "--mfma16", "fp4", "--vmem", "buf")
    assert rc == 0 and res["ok"], (r.stdout, r.stderr)
    assert res["sparse"]["i8"]["ok"] is True and res["sparse"]["i8"]["errors"] == 0, res["sparse"]
    for word in ("lds", "mfma16", "vmem"):
        assert res[word]["ok"] is True and res[word]["errors"] == 0 and res[word]["bad"] == "", res[word]
    assert not {"mx", "dtypes", "fp", "cvt"} & set(res)
