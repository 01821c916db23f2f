"""The LDS step of the start-up probe and the transposer of packed codes, without a GPU.

* the controller: the ``lds`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_LDS``, with every value
  accepted before producing the arguments it produced;
* ``odh-gpu-probe --lds``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants and signatures against ``gpu_probe.h``;
* ``odh_lds_cases`` and ``odh_lds_fault_count`` of the built library against the host model
  (``lds_reference.py``) for every check and every table byte;
* properties of the model: the lane maps are bijections, the ``mem`` passes toggle every bit, the 4- and 6-bit
  rounds tell any two positions of a block apart, the transposer's LDS layouts are conflict-free by the bank
  rule, transposing twice is the identity.
"""

from __future__ import annotations

import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lds_reference as lr
from odh_kubeflow_amd.controllers import notebook as nbc
from odh_kubeflow_amd.controllers.notebook import (GPU_PROBE_ANNOTATION, GPU_PROBE_CONTAINER, generate_statefulset)
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.ops import gpu, probe_main

torch = pytest.importorskip("torch")

# ------------------------------------------------------------------ controller


def _args(value=None, env=None, gpus=2):
    nb = notebook("nb", "ns", gpus=gpus, annotations={GPU_PROBE_ANNOTATION: value} if value is not None else None)
    inits = generate_statefulset(nb, False, env or {})["spec"]["template"]["spec"].get("initContainers") or []
    assert [c["name"] for c in inits] in ([], [GPU_PROBE_CONTAINER])
    return inits[0]["args"] if inits else None


BASE = ["--json", "/dev/termination-log", "--timeout-ms", "30000"]
RCCL = ["--rccl-mib", "64"]
MX = ["--mx", "fp8,fp4"]
MX_ALL = ["--mx", "fp8,fp4,bf8,fp6,bf6"]
DTYPES = ["--dtypes", "f16,i8"]
FP = ["--fp", "f32,f64"]
SPARSE = ["--sparse", "bf16,f16,i8,fp8,bf8"]
CVT = ["--cvt", "fp8,bf8,fp4,fp6,bf6,bf16"]
LDS = ["--lds", "mem,tr16,tr8,tr4,tr6,xlane"]


def test_lds_token_adds_the_step_after_the_others():
    assert nbc.GPU_PROBE_LDS_FORMATS == "mem,tr16,tr8,tr4,tr6,xlane" == ",".join(gpu.LDS_CHECKS) == ",".join(lr.NAMES)
    assert nbc.GPU_PROBE_LDS_TOKENS == ("lds",)
    assert "lds" not in (nbc.GPU_PROBE_TOKENS + nbc.GPU_PROBE_MORE_TOKENS + nbc.GPU_PROBE_SPARSE_TOKENS
                         + nbc.GPU_PROBE_CVT_TOKENS)
    assert nbc.GPU_PROBE_CVT_TOKENS == ("cvt",)
    assert _args("lds") == BASE + LDS
    assert _args("lds", gpus=1) == BASE + LDS
    assert _args("true,lds") == BASE + LDS
    assert _args("rccl,mxall,dtypes,fp,sparse,cvt,lds") == BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE + CVT + LDS
    assert _args(" LDS , dtypes,rccl ") == BASE + RCCL + DTYPES + LDS
    others = {"rccl": RCCL, "mx": MX, "mxall": MX_ALL, "dtypes": DTYPES, "fp": FP, "sparse": SPARSE, "cvt": CVT}
    for r in range(len(others) + 1):
        for subset in itertools.combinations(others, r):
            want = list(BASE)
            for token in ("rccl", "mxall" if "mxall" in subset else "mx", "dtypes", "fp", "sparse", "cvt"):
                if token in subset:
                    want += others[token]
            assert _args(",".join(subset + ("lds",))) == want + LDS, subset
            assert _args(",".join(("lds",) + subset)) == want + LDS, subset
            if subset:
                assert _args(",".join(subset)) == want, subset  # and without it, what it was


def test_operator_switch_adds_lds_to_every_probed_notebook():
    on = {"GPU_PROBE_LDS": "true"}
    assert _args("true", on) == BASE + LDS
    assert _args("rccl", on) == BASE + RCCL + LDS
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + LDS
    assert _args(None, on) is None  # it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("mx", dict(on, GPU_PROBE_CVT="true", GPU_PROBE_DTYPES="true")) == BASE + MX + DTYPES + CVT + LDS
    assert _args("lds", {"GPU_PROBE_LDS": "false"}) == BASE + LDS


def test_unknown_token_ignores_the_whole_value():
    for value in ("lds,bogus", "false,lds", "lds,", "lds_", "ld", "shared"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


@pytest.mark.parametrize("lds_on", [False, True])
def test_values_accepted_before_keep_their_args(lds_on):
    """Every value the earlier steps' tests list, with the arguments they list for it; under
    ``GPU_PROBE_LDS=true`` each probed one gains ``--lds`` at the end."""
    on = {"GPU_PROBE_LDS": "true"} if lds_on else {}

    def check(value, env, want, **kw):
        assert _args(value, dict(env, **on), **kw) == (want + LDS if lds_on and want is not None else want), \
            (value, env)

    startup = {"GPU_STARTUP_PROBE": "true"}
    check("true", {}, BASE)
    check("rccl", {}, BASE + RCCL)
    check("false", startup, None)
    check(None, {}, None)
    check(None, startup, BASE)
    check("mx", {}, BASE + MX)
    check("rccl,mx", {}, BASE + RCCL + MX)
    check(" MX , rccl ", {}, BASE + RCCL + MX)
    check("true,mx", {}, BASE + MX)
    check("mx", {}, BASE + MX, gpus=1)
    mx_on = {"GPU_PROBE_MX": "true"}
    check("true", mx_on, BASE + MX)
    check(None, dict(mx_on, **startup), BASE + MX)
    check(None, mx_on, None)
    for value in ("mx,bogus", "yes", "mx,", "false,mx", "dtypes,bogus", "false,dtypes", "dtype", "fp,bogus", "fp32",
                  "sparse,bogus", "false,sparse", "sparse,", "sparsity", "smfmac", "cvt,bogus", "false,cvt", "cvt,",
                  "convert", "cvts"):
        check(value, {}, None)
        check(value, startup, BASE)
    check("dtypes", {}, BASE + DTYPES)
    check("rccl,mx,dtypes", {}, BASE + RCCL + MX + DTYPES)
    check("mxall", {}, BASE + MX_ALL)
    check("mx,mxall,dtypes", {}, BASE + MX_ALL + DTYPES)
    dt_on = {"GPU_PROBE_DTYPES": "true"}
    check("true", dt_on, BASE + DTYPES)
    check("mx", dict(dt_on, **mx_on), BASE + MX + DTYPES)
    check("true", {"GPU_PROBE_MX_ALL": "true"}, BASE + MX_ALL)
    check("true", {"GPU_PROBE_RCCL": "true"}, BASE + RCCL)
    check("true", {"GPU_PROBE_RCCL": "true"}, BASE, gpus=1)
    check("fp", {}, BASE + FP)
    check("rccl,mxall,dtypes,fp", {}, BASE + RCCL + MX_ALL + DTYPES + FP)
    check("true", {"GPU_PROBE_FP": "true"}, BASE + FP)
    check("mx", dict(dt_on, GPU_PROBE_FP="true"), BASE + MX + DTYPES + FP)
    check("sparse", {}, BASE + SPARSE)
    check("rccl,mxall,dtypes,fp,sparse", {}, BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE)
    check("true", {"GPU_PROBE_SPARSE": "true"}, BASE + SPARSE)
    check("mx", dict(dt_on, GPU_PROBE_FP="true", GPU_PROBE_SPARSE="true"), BASE + MX + DTYPES + FP + SPARSE)
    check("cvt", {}, BASE + CVT)
    check("rccl,mxall,dtypes,fp,sparse,cvt", {}, BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE + CVT)
    check("true", {"GPU_PROBE_CVT": "true"}, BASE + CVT)


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_LDS=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_LDS=false\n" in f.read()


# ------------------------------------------------------------------ the program


def _exe():
    path = probe_main.executable()
    if not os.path.exists(path):
        pytest.fail("odh-gpu-probe not built: python -m odh_kubeflow_amd.ops.build")
    return path


def _run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # a pod without GPUs (also on a GPU machine)
    return subprocess.run([_exe(), "--json", "-", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args", [
    ("--lds", "bogus"), ("--lds", "mem,bogus"), ("--lds", "tr32"), ("--lds", "fp8"), ("--lds", ""), ("--lds", "mem,"),
    ("--lds", "mem,mem"), ("--lds", "tr4,xlane,tr4"), ("--lds",),
    ("--inject-fault", "lds"), ("--cvt", "bf16", "--inject-fault", "lds"), ("--inject-fault", "lane")])
def test_program_lds_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert "[--lds mem,tr16,tr8,tr4,tr6,xlane]" in r.stderr and "[--inject-fault lds]" in r.stderr
    assert "[--cvt fp8,bf8,fp4,fp6,bf6,bf16]" in r.stderr and "[--sparse bf16,f16,i8,fp8,bf8]" in r.stderr
    assert "rccl|mx|dtypes|fp]" in r.stderr and "[--inject-fault sparse]" in r.stderr
    assert "[--inject-fault cvt]" in r.stderr


def test_program_no_gpu_verdict_with_lds():
    r = _run("--lds", "mem,tr16,tr8,tr4,tr6,xlane")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "lds" not in res
    # accepted next to the other steps, in any order, one check alone, and with its fault hook
    assert _run("--lds", "xlane,mem", "--mx", "fp8,fp4", "--cvt", "bf16").returncode == probe_main.NO_GPU
    assert _run("--sparse", "fp8,bf16", "--dtypes", "f16,i8", "--mx", "fp8,fp4,bf8,fp6,bf6", "--fp", "f32,f64",
                "--cvt", "fp6", "--lds", "tr6", "--inject-fault", "lds").returncode == probe_main.NO_GPU
    assert _run("--lds=tr8", "--inject-fault=lds").returncode == probe_main.NO_GPU
    # the step uses no operand: it puts no condition on the shape
    assert _run("--lds", "mem", "--shape", "256,256,64").returncode == probe_main.NO_GPU


# ------------------------------------------------------------------ ABI mirror


def test_constants_and_signatures_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        text = f.read()
    header = {k: int(v) for k, v in re.findall(r"^\s*(ODH_(?:LDS|TC)_\w+)\s*=\s*(\d+)\s*,", text, re.M)}
    assert header == {"ODH_LDS_MEM": 0, "ODH_LDS_TR16": 1, "ODH_LDS_TR8": 2, "ODH_LDS_TR4": 3, "ODH_LDS_TR6": 4,
                      "ODH_LDS_XLANE": 5, "ODH_LDS_BLOCKS": 256, "ODH_LDS_TABLE": 1024, "ODH_LDS_CU_WORDS": 64,
                      "ODH_LDS_TR_RAW": 256, "ODH_TC_B16": 0, "ODH_TC_B8": 1, "ODH_TC_B4": 2, "ODH_TC_B6": 3}
    for name, value in header.items():
        assert getattr(gpu, name) == value, name
    assert gpu.LDS_CHECKS == lr.NAMES and (lr.BLOCKS, lr.TABLE) == (gpu.ODH_LDS_BLOCKS, gpu.ODH_LDS_TABLE)
    assert gpu.LDS_XLANE_OPS == lr.OPS and gpu.LDS_XLANE_ARGS == lr.ARGS
    assert {f: b for f, (_, b) in gpu.TRANSPOSE_FORMATS.items()} == lr.FORMAT_BITS
    params = {"odh_lds_cases": 1, "odh_lds_fault_count": 2, "odh_lds_fill": 3, "odh_lds_probe_verify": 4,
              "odh_lds_tr_read": 6, "odh_lds_xlane": 5, "odh_transpose_codes": 6}
    for name, n in params.items():
        assert len(gpu.SIGNATURES[name][1]) == n, name
        assert re.search(r"\b%s\(" % name, text), name


def test_entry_points_check_their_arguments_before_anything_else():
    for bad in ("tr32", "lds", "fp8", 6, -1, True):
        for fn in (gpu.lds_cases, lambda c: gpu.lds_fault_count(c, 0)):
            with pytest.raises(ValueError):
                fn(bad)
    for byte in (-1, 1024):
        with pytest.raises(ValueError):
            gpu.lds_fault_count("mem", byte)
    lib = gpu.load_library()
    assert lib.odh_lds_cases(6) == 0 and lib.odh_lds_cases(-1) == 0
    assert lib.odh_lds_fault_count(6, 0) == 0 and lib.odh_lds_fault_count(0, 1024) == 0 == lib.odh_lds_fault_count(0, -1)
    # a bad check, op, selector or shape is refused before a pointer is looked at, let alone a launch
    invalid = 1  # hipErrorInvalidValue
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()
    assert lib.odh_lds_fill(6, p, None) == invalid and lib.odh_lds_fill(0, None, None) == invalid
    assert lib.odh_lds_probe_verify(-1, p, p, None) == invalid and lib.odh_lds_probe_verify(0, p, None, None) == invalid
    assert lib.odh_lds_tr_read(0, p, 256, p, p, None) == invalid  # mem is no transposing read
    assert lib.odh_lds_tr_read(5, p, 256, p, p, None) == invalid
    assert lib.odh_lds_tr_read(1, p, 65540, p, p, None) == invalid and lib.odh_lds_tr_read(1, p, 0, p, p, None) == invalid
    assert lib.odh_lds_xlane(8, 0, p, p, None) == invalid and lib.odh_lds_xlane(-1, 0, p, p, None) == invalid
    for op, n in enumerate(lr.ARGS.values()):
        assert lib.odh_lds_xlane(op, n, p, p, None) == invalid and lib.odh_lds_xlane(op, -1, p, p, None) == invalid
    for fmt, r, c in ((4, 128, 128), (-1, 128, 128), (0, 64, 128), (0, 128, 64), (1, 0, 128), (2, 128, -128),
                      (3, 192, 128)):
        assert lib.odh_transpose_codes(fmt, p, p, r, c, None) == invalid, (fmt, r, c)
    assert not buf.any()
    # tensors that are not on a GPU are refused before the library is asked
    t = torch.zeros(gpu.ODH_LDS_TABLE, dtype=torch.uint8)
    for fn in (lambda: gpu.lds_fill("mem", t), lambda: gpu.lds_verify("mem", t),
               lambda: gpu.lds_tr_read("tr8", torch.zeros(256, dtype=torch.uint8), [0] * 64),
               lambda: gpu.lds_xlane("dpp", 0, torch.zeros(64, dtype=torch.int32)),
               lambda: gpu.transpose_codes("fp8", torch.zeros((128, 128), dtype=torch.uint8)),
               lambda: gpu.transpose_codes("fp5", torch.zeros((128, 128), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            fn()


# ------------------------------------------------------------------ counts


@pytest.mark.parametrize("name", list(lr.NAMES))
def test_library_counts_are_the_models(name):
    check = lr.NAMES[name]
    assert gpu.lds_cases(name) == lr.cases(check) > 0
    lib = gpu.load_library()
    got = [lib.odh_lds_fault_count(check, b) for b in range(lr.TABLE)]
    assert got == [lr.fault_count(check, b) for b in range(lr.TABLE)]
    assert min(got) > 0  # no table byte is unused: a wrong one always shows
    assert sum(got[::4]) == lr.cases(check)  # every compared element uses exactly one key dword


def test_case_counts_of_the_construction():
    assert lr.cases(lr.MEM) == 160 * 1024 // 4 * 4 * 256  # every dword, four passes, every workgroup
    for check, rounds, elements in ((lr.TR16, 96, 16 * 64), (lr.TR8, 96, 32 * 64), (lr.TR4, 96, 64 * 64),
                                    (lr.TR6, 48, 64 * 64)):
        assert lr.tr_geometry(check)["rounds"] == rounds
        assert lr.cases(check) == rounds * elements * 4 * 4 * 256  # to each group of lanes of each wave
    per_repeat = sum(64 * n for n in lr.ARGS.values()) + 64 * 8  # the swaps compare both registers
    assert lr.cases(lr.XLANE) == per_repeat * lr.XL_REPEAT * 4 * 256


def test_fold_takes_any_change_of_a_byte_where_an_element_is_wide_enough():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    for delta in range(1, 256):
        for byte in range(4):
            changed = keys ^ (delta << (8 * byte))
            for bits in (32, 16, 8):
                assert (lr.fold(changed, bits) != lr.fold(keys, bits)).all()
            same_nibbles = (delta ^ (delta >> 4)) & 15 == 0
            assert (lr.fold(changed, 4) != lr.fold(keys, 4)).all() != same_nibbles
            assert lr.fold_changes(lr.TR4, delta) != same_nibbles and lr.fold_changes(lr.TR8, delta)
    assert lr.fold_changes(lr.TR6, 1) and not lr.fold_changes(lr.TR6, 0x11)


# ------------------------------------------------------------------ properties of the model


def test_mem_passes_toggle_every_bit_and_no_wave_reads_its_own():
    w = np.arange(lr.MEM_DWORDS)
    ones = np.zeros(lr.MEM_DWORDS, dtype=np.uint64)
    zeros = np.zeros(lr.MEM_DWORDS, dtype=np.uint64)
    for p in range(lr.MEM_PASSES):
        v = lr.mem_values(p)
        ones |= v
        zeros |= ~v & lr.M32
    assert (ones == lr.M32).all() and (zeros == lr.M32).all()
    assert np.array_equal(lr.mem_values(1), ~lr.mem_values(0) & lr.M32)
    assert not np.array_equal(lr.mem_values(2), lr.mem_values(0))
    assert (lr.mem_reader_wave(w) != lr.mem_writer_wave(w)).all()
    # every wave reads a quarter, from each of the three others
    for v in range(4):
        mine = lr.mem_reader_wave(w) == v
        assert mine.sum() == lr.MEM_DWORDS // 4
        assert set(lr.mem_writer_wave(w[mine]).tolist()) == {0, 1, 2, 3} - {v}


@pytest.mark.parametrize("name", ["tr16", "tr8", "tr4", "tr6"])
def test_lane_map_is_a_bijection_of_bits(name):
    """An image whose every bit is its own address: four disjoint blocks at a pitch of 80 bytes, read by the four
    groups; the result bits are exactly the blocks' bits, each once."""
    check = lr.NAMES[name]
    bits, rows, _, slot, width = lr.TR[check]
    pitch = 80
    image = np.zeros(4 * rows * pitch + 64, dtype=np.uint8)
    addr = [g * rows * pitch + lr.tr_lane_offset(check, i, pitch) for g in range(4) for i in range(16)]
    # tag bit b of the image by reading with one bit set at a time would be slow: read bit planes of the address
    nbits = image.size * 8
    planes = int(np.ceil(np.log2(nbits)))
    idx = np.arange(nbits)
    got = np.zeros((64, width * 8), dtype=np.int64)
    for k in range(planes):
        img = np.packbits(((idx >> k) & 1).astype(np.uint8), bitorder="little")
        out = np.unpackbits(lr.tr_read(check, img, addr), axis=1, bitorder="little")
        got |= out.astype(np.int64) << k
    want = set()
    for g in range(4):
        for q in range(rows):
            first = (g * rows + q) * pitch * 8
            want |= set(range(first, first + 16 * bits))
    assert len(set(got.ravel().tolist())) == got.size == 64 * width * 8 == len(want)
    assert set(got.ravel().tolist()) == want
    # lane i of a group holds column i: element q of lane 16 g + i is bit-contiguous and starts at row q, column i
    for lane in (0, 5, 15, 16, 37, 63):
        g, i = divmod(lane, 16)
        for q in range(rows):
            e = got[lane, bits * q:bits * q + bits]
            assert (np.diff(e) == 1).all() and e[0] == (g * rows + q) * pitch * 8 + i * bits, (lane, q)


@pytest.mark.parametrize("name", ["tr4", "tr6"])
def test_narrow_rounds_separate_any_two_positions_of_a_block(name):
    """4- and 6-bit values cannot be unique in a block of 256; over the rounds any two positions of a block differ
    in at least one, so a swap of any two is caught."""
    check = lr.NAMES[name]
    g = lr.tr_geometry(check)
    v = np.stack([lr.tr_values(check, rnd) for rnd in range(g["rounds"])])  # [round, row, col]
    for rb in range(4):
        for cb in range(4):
            blk = v[:, rb * g["block_rows"]:(rb + 1) * g["block_rows"], 16 * cb:16 * cb + 16].reshape(g["rounds"], -1)
            same = (blk[:, :, None] == blk[:, None, :]).all(axis=0)
            assert same.sum() == blk.shape[1], (rb, cb)  # only the diagonal


@pytest.mark.parametrize("name", ["tr16", "tr8", "tr4", "tr6"])
def test_rounds_visit_every_position_and_three_pitches(name):
    check = lr.NAMES[name]
    g = lr.tr_geometry(check)
    rounds = range(g["rounds"])
    pitches = sorted({lr.tr_pitch(check, r) for r in rounds})
    assert len(pitches) == 3 and any(p & (p - 1) for p in pitches) and all(p % g["align"] == 0 for p in pitches)
    for p in pitches:
        assert {lr.tr_base(check, r) for r in rounds if lr.tr_pitch(check, r) == p} == set(range(0, 256, g["align"]))
    for read in range(16):
        assert len({lr.tr_block_of(grp, read) for grp in range(4)}) == 4  # the groups read different blocks
    for grp in range(4):
        assert len({lr.tr_block_of(grp, read) for read in range(16)}) == 16
    # the model's instruction on the model's image gives the model's values
    img, base, pitch = lr.tr_image(check, 7)
    rb, cb = 2, 1
    addr = [base + rb * g["block_rows"] * pitch + cb * g["slot"] + lr.tr_lane_offset(check, i, pitch)
            for _ in range(4) for i in range(16)]
    got = lr.tr_unpack(check, lr.tr_read(check, img, addr))
    want = lr.tr_values(check, 7)[rb * g["block_rows"]:(rb + 1) * g["block_rows"], 16 * cb:16 * cb + 16].T
    assert np.array_equal(got[:16], want) and np.array_equal(got[48:], want)


def test_exchanges_cover_what_the_step_promises():
    for name in ("bpermute", "permute"):
        rot = [lr.xl_sources(name, a) for a in range(64)]
        assert all(sorted(s.tolist()) == list(range(64)) for s in rot)
        assert len({tuple(s.tolist()) for s in rot}) == 64  # all 64 rotations
        rev = lr.xl_sources(name, 64)
        assert sorted(rev.tolist()) == list(range(64)) and rev[1] == 32 and rev[3] == 48
    assert np.array_equal(lr.xl_sources("bpermute", 5), (np.arange(64) + 5) % 64)
    assert np.array_equal(lr.xl_sources("permute", 5), (np.arange(64) - 5) % 64)
    kinds = [lr.xl_sources("swizzle", a) for a in range(lr.ARGS["swizzle"])]
    assert np.array_equal(kinds[0], np.arange(64) ^ 1) and np.array_equal(kinds[4], np.arange(64) ^ 16)  # swap
    assert np.array_equal(kinds[5], np.arange(64) ^ 31)  # reverse
    assert (kinds[8][:32] == 0).all() and (kinds[8][32:] == 32).all()  # broadcast
    assert {lr.DPP[a] for a in range(lr.ARGS["dpp"])} >= set(range(0x101, 0x110)) | set(range(0x111, 0x120)) \
        | set(range(0x121, 0x130)) | {0x140, 0x141, 0x142, 0x143}
    assert np.array_equal(lr.xl_sources("dpp", lr.DPP.index(0x111))[:17], [0] + list(range(15)) + [16])  # row_shr:1
    assert [lr.xl_sources("readlane", a).tolist() for a in range(64)] == [[a] * 64 for a in range(64)]
    for a in range(64):
        s = lr.xl_sources("writelane", a)
        assert s[a] == (a + 1) % 64 and (np.delete(s, a) == np.delete(np.arange(64), a)).all()
    for name in ("permlane16_swap", "permlane32_swap"):
        for a in range(4):
            s = lr.xl_sources(name, a)
            assert sorted(s.tolist()) == list(range(128)) and (s != np.arange(128)).sum() == 64
    assert len(lr.xl_exchanges()) == sum(lr.ARGS.values())


@pytest.mark.parametrize("fmt", list(lr.FORMAT_BITS))
def test_transpose_twice_is_the_identity(fmt):
    rng = np.random.default_rng(11)
    bits = lr.FORMAT_BITS[fmt]
    r, c = 128, 384
    x = rng.integers(0, 1 << 16, (r, c), dtype=np.uint16) if bits == 16 \
        else rng.integers(0, 256, (r, c * bits // 8), dtype=np.uint8)
    t = lr.transpose_codes(fmt, x)
    assert t.shape == ((c, r) if bits == 16 else (c, r * bits // 8)) and t.dtype == x.dtype
    assert np.array_equal(lr.unpack_codes(fmt, t), lr.unpack_codes(fmt, x).T)
    assert np.array_equal(lr.transpose_codes(fmt, t), x)
    assert not np.array_equal(t[:128, :x.shape[1]], x[:, :t.shape[1]][:128])


@pytest.mark.parametrize("bits", [16, 8, 4, 6])
def test_transposer_lds_layout_is_conflict_free_by_the_bank_rule(bits):
    reads = lr.tc_read_addresses(bits)
    check, pitch, row = lr.TC[bits]
    _, rows, align, _, width = lr.TR[check]
    assert all(a % align == 0 and a + width <= 128 * pitch for *_, addr in reads for a in addr)
    assert lr.tc_read_conflicts(bits) == 0 and lr.tc_write_conflicts(bits) == 0
    # every block of the tile is read exactly once
    seen = [(a[0], a[16], a[32], a[48]) for *_, a in reads]
    firsts = [x for t in seen for x in t]
    assert len(set(firsts)) == len(firsts) == (128 // rows) * 8
    # the rule does find conflicts: the same reads on the unpadded pitch
    lr.TC[bits] = (check, row, row)
    try:
        assert lr.tc_read_conflicts(bits) > 0
    finally:
        lr.TC[bits] = (check, pitch, row)
