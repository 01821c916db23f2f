"""The decoding converters on the MI355X: one instruction at a time, ``mx_dequantize`` against a float64 decode
table, the fused check, and the program's ``--dcvt`` step.  The reference is ``mx_reference.code_values`` (every code's
value from the format definition) times ``2.0 ** (byte - 127)``, cast by numpy / torch to the destination."""

import json

import numpy as np
import pytest
import torch

import mx_reference as ref
from probe_gpu import _run_probe
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)
from odh_kubeflow_amd.ops import gpu

pytestmark = pytest.mark.gpu

FORMATS = list(gpu.DCVT_FORMATS)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# the exact windows, scale bytes lo … hi (bf8 has none in float16), from the issue's two bounds
WINDOW = {("fp8", 32): (10, 246), ("fp8", 16): (122, 134), ("bf8", 32): (17, 239), ("bf8", 16): None,
          ("fp4", 32): (2, 252), ("fp4", 16): (114, 140), ("fp6", 32): (4, 252), ("fp6", 16): (116, 140),
          ("bf6", 32): (5, 250), ("bf6", 16): (117, 138)}


def _bits(values, dtype):
    """float64 ``values`` cast to ``dtype`` (round to nearest even), as integers, and where they are NaN."""
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(over="ignore"):
        if dtype == torch.bfloat16:  # every product here is exact in float32 or overflows it, so this rounds once
            b = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy()
        else:
            b = v.astype(np.float32).view(np.int32) if dtype == torch.float32 else v.astype(np.float16).view(np.int16)
    return b.astype(np.int64), np.isnan(v)


def _same(got, values, dtype):
    want, nan = _bits(values, dtype)
    got = got.view(torch.int32 if dtype == torch.float32 else torch.int16).cpu().numpy().astype(np.int64).reshape(want.shape)
    mag = 0x7FFFFFFF if dtype == torch.float32 else 0x7FFF
    inf = {torch.float32: 0x7F800000, torch.float16: 0x7C00, torch.bfloat16: 0x7F80}[dtype]
    assert ((got & mag) > inf)[nan].all(), "a NaN is expected"
    bad = np.flatnonzero(((got != want) & ~nan).ravel())
    assert bad.size == 0, (bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


# the packed instruction of every format to every destination, and the one-value form there is
ONE = [(f, d, 0) for f in FORMATS for d in DTYPES] + [("fp8", torch.float32, 1), ("bf8", torch.float32, 1)]


@pytest.mark.parametrize("fmt, dtype, form", ONE, ids=lambda v: str(v).replace("torch.", ""))
def test_one_instruction_equals_the_table(dev, fmt, dtype, form):
    table = ref.code_values(ref.NAMES[fmt])
    window = WINDOW[fmt, 16 if dtype == torch.float16 else 32]
    lanes = np.arange(64)
    for byte in sorted({127} | set(window or ())):
        scale = torch.full((64,), byte << 23, dtype=torch.int32, device=dev)
        if fmt in ("fp6", "bf6"):  # code (l + k) & 63 at position k of lane l: every code in every position
            codes = (lanes[:, None] + np.arange(32)) & 63
            src = torch.from_numpy(ref.pack6(codes)).to(dev).view(torch.int32)
            _same(gpu.dcvt_one(fmt, dtype, src, scale), table[codes] * 2.0 ** (byte - 127), dtype)
            continue
        for t in range(4):  # byte value 64 t + l in position 0 of lane l, other values in the other positions
            by = (64 * t + lanes[:, None] + 85 * np.arange(4)) & 255
            src = torch.from_numpy((by << (8 * np.arange(4))).sum(axis=1).astype(np.uint32).view(np.int32)).to(dev)
            for sel in range(4 if fmt == "fp4" or form == 1 else 2):
                if fmt == "fp4":
                    codes = np.stack([by[:, sel] & 15, by[:, sel] >> 4], axis=1)
                else:
                    codes = by[:, sel:sel + 1] if form == 1 else by[:, 2 * sel:2 * sel + 2]
                _same(gpu.dcvt_one(fmt, dtype, src, scale, sel=sel, form=form), table[codes] * 2.0 ** (byte - 127), dtype)


def _random_case(fmt, rows, k, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (rows, gpu.mx_row_bytes(fmt, k)), dtype=np.uint8)
    scales = rng.integers(0, 255, (rows, k // 32), dtype=np.uint8)
    scales.reshape(-1)[15::16] = 255  # the E8M0 NaN in exactly one block of every 16
    values = ref.decode(ref.NAMES[fmt], codes) * np.repeat(2.0 ** (scales.astype(np.float64) - 127), 32, axis=1)
    values[np.repeat(scales == 255, 32, axis=1)] = np.nan
    return codes, scales, values


@pytest.mark.parametrize("rows, k", [(1, 32), (5, 160), (1031, 64)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_dequantize_equals_the_reference(dev, fmt, dtype, rows, k):
    codes, scales, values = _random_case(fmt, rows, k, seed=rows)
    assert np.isnan(values).mean() <= 1 / 16 + 6 / 256
    out = gpu.mx_dequantize(fmt, torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev), dtype)
    assert out.dtype == dtype and tuple(out.shape) == (rows, k)
    _same(out, values, dtype)


@pytest.mark.parametrize("fmt", FORMATS)
def test_dequantize_inverts_quantize(dev, fmt):
    rng = np.random.default_rng(7)
    finite = ref.code_values(ref.NAMES[fmt])
    finite = finite[np.isfinite(finite) & (finite != 0)]
    x = rng.choice(finite, (3, 96))
    x.reshape(-1, 32)[:, 0] = finite.max()  # the block's amax, so its scale is the power of two below
    x = (x.reshape(-1, 32) * 2.0 ** rng.integers(-20, 21, (9, 1))).reshape(3, 96)
    xt = torch.from_numpy(x.astype(np.float32)).to(dev)
    assert (xt.double().cpu().numpy() == x).all()
    assert torch.equal(gpu.mx_dequantize(fmt, *gpu.mx_quantize(fmt, xt)), xt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_check_clean_and_with_one_table_byte_flipped(dev, fmt):
    r = gpu.dcvt_probe(0, fmt)
    print(fmt, r)
    assert r["errors"] == 0 and r["xcd_blocks"] == [gpu.ODH_CVT_BLOCKS // gpu.ODH_N_XCD] * gpu.ODH_N_XCD, r
    table = torch.empty(gpu.ODH_CVT_TABLE, dtype=torch.uint8, device=dev)
    gpu.dcvt_fill(fmt, table)
    for byte, flip in ((9, 0x01), (120, 0x10)):  # the second scale lies in float16's window too
        want = gpu.dcvt_fault_count(fmt, byte)
        table[byte] ^= flip
        r = gpu.dcvt_verify(fmt, table)
        table[byte] ^= flip
        assert want > 0 and r["errors"] == want and sum(r["err_xcd"]) == want, (byte, want, r)


def test_entry_point_checks_before_launch(dev):
    codes, scales = torch.zeros((2, 64), dtype=torch.uint8, device=dev), torch.full((2, 2), 127, dtype=torch.uint8, device=dev)
    for bad in [lambda: gpu.mx_dequantize("bf16", codes, scales), lambda: gpu.mx_dequantize("fp8", codes, scales[:1]),
                lambda: gpu.mx_dequantize("fp8", codes, scales, torch.float64),
                lambda: gpu.mx_dequantize("fp6", codes, scales), lambda: gpu.mx_dequantize("fp8", codes[:, :48], scales)]:
        with pytest.raises(ValueError):
            bad()
    lib, out = gpu.load_library(), torch.zeros((2, 64), dtype=torch.float32, device=dev)
    for args in [(9, 0, codes.data_ptr(), scales.data_ptr(), out.data_ptr(), 2, 64), (0, 3, codes.data_ptr(), scales.data_ptr(), out.data_ptr(), 2, 64),
                 (0, 0, codes.data_ptr() + 4, scales.data_ptr(), out.data_ptr(), 1, 32), (0, 0, codes.data_ptr(), scales.data_ptr(), out.data_ptr() + 8, 1, 32),
                 (0, 0, codes.data_ptr(), scales.data_ptr(), out.data_ptr(), 2, 48), (0, 0, codes.data_ptr(), scales.data_ptr(), out.data_ptr(), 1 << 34, 64)]:
        assert lib.odh_mx_dequantize(*args, 0) != 0
    torch.cuda.synchronize()
    assert not out.any()


EVERY = {"mx": "fp8,fp4,bf8,fp6,bf6", "dtypes": "f16,i8", "fp": "f32,f64", "sparse": "bf16,f16,i8,fp8,bf8",
         "cvt": "fp8,bf8,fp4,fp6,bf6,bf16", "lds": "mem,tr16,tr8,tr4,tr6,xlane", "mfma16": "bf16,f16,i8,fp8,fp4",
         "vmem": "cache,sub,buf,dma", "dcvt": "fp8,bf8,fp4,fp6,bf6"}


def test_program_runs_the_step_and_names_the_faulted_format():
    from odh_kubeflow_amd.ops import probe_main

    rc, res, r = _run_probe("--dcvt", EVERY["dcvt"])
    assert rc == 0 and res["ok"], (r.stdout, r.stderr)
    assert res["dcvt"]["ok"] is True and res["dcvt"]["errors"] == 0 and res["dcvt"]["bad"] == "" and res["dcvt"]["ms"] > 0
    assert list(res)[-3:] == ["dcvt", "setup_ms", "timings_ms"] and list(res["timings_ms"])[-2:] == ["dcvt", "total"]
    assert len(r.stdout.strip().splitlines()[-1].encode()) < 4096
    print("dcvt:", res["dcvt"], res["timings_ms"])
    rc, res, r = _run_probe("--dcvt", "bf6,fp8", "--inject-fault", "dcvt")
    assert rc == probe_main.CHECK_FAILED and res["ok"] is False, (r.stdout, r.stderr)
    assert res["dcvt"]["bad"] == "bf6" and res["dcvt"]["errors"] == gpu.dcvt_fault_count("bf6", 3), res["dcvt"]
    assert "dcvt bf6" in res["error"] and res["results"][0]["ok"] is True


@pytest.mark.parametrize("fault", [None, "dcvt"])
def test_every_step_still_gives_whole_json_under_4096_bytes(fault):
    args = ["--rccl-mib", "16"] + [a for word, formats in EVERY.items() for a in ("--" + word, formats)]
    rc, res, r = _run_probe(*args, *(["--inject-fault", fault] if fault else []))
    line = r.stdout.strip().splitlines()[-1]
    print("every step, fault", fault, ":", len(line), "bytes")
    assert json.loads(line) == res and len(line.encode()) < 4096
    assert (rc == 0 and res["ok"]) if fault is None else (rc != 0 and not res["ok"] and "dcvt fp8" in res["error"])
    assert [k for k in res if k in EVERY] == list(EVERY) and res["rccl"]["ok"] is True
    for word, formats in EVERY.items():
        entries = [res[word]] if "bad" in res[word] else [res[word][f] for f in formats.split(",")]
        assert all(e["ok"] is (word != fault) for e in entries), (word, res[word])
