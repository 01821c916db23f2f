"""The 2:4 structured-sparsity step of the start-up probe, without a GPU.

* the controller: the ``sparse`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_SPARSE``, with every
  value accepted before producing the arguments it produced;
* ``odh-gpu-probe --sparse``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants against ``gpu_probe.h``;
* the host model (``sparse_reference.py``): the 30 × 7 table against the full product of the pruned
  operands, the properties of the family, ``odh_sparse_zero_classes``, the exactness bounds;
* ``sparse_compress`` / ``sparse_decompress`` of ``ops/gpu.py`` on CPU tensors.
"""

from __future__ import annotations

import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import probe_reference as ref
import sparse_reference as sp
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


def test_sparse_token_adds_the_step_after_the_others():
    assert nbc.GPU_PROBE_SPARSE_FORMATS == "bf16,f16,i8,fp8,bf8"
    assert "sparse" in nbc.GPU_PROBE_TOKENS + nbc.GPU_PROBE_MORE_TOKENS + nbc.GPU_PROBE_SPARSE_TOKENS
    assert _args("sparse") == BASE + SPARSE
    assert _args("sparse", gpus=1) == BASE + SPARSE
    assert _args("true,sparse") == BASE + SPARSE
    assert _args("rccl,mxall,dtypes,fp,sparse") == BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE
    assert _args(" SPARSE , dtypes,rccl ") == BASE + RCCL + DTYPES + SPARSE
    others = {"rccl": RCCL, "mx": MX, "mxall": MX_ALL, "dtypes": DTYPES, "fp": FP}
    for r in range(len(others) + 1):
        for subset in itertools.combinations(others, r):
            want = list(BASE)
            for token in ("rccl", "mxall" if "mxall" in subset else "mx", "dtypes", "fp"):
                if token in subset:
                    want += others[token]
            assert _args(",".join(subset + ("sparse",))) == want + SPARSE, subset
            assert _args(",".join(("sparse",) + subset)) == want + SPARSE, subset
            if subset:
                assert _args(",".join(subset)) == want, subset  # and without it, what it was


def test_operator_switch_adds_sparse_to_every_probed_notebook():
    on = {"GPU_PROBE_SPARSE": "true"}
    assert _args("true", on) == BASE + SPARSE
    assert _args("rccl", on) == BASE + RCCL + SPARSE
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + SPARSE
    assert _args(None, on) is None  # it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("mx", dict(on, GPU_PROBE_FP="true", GPU_PROBE_DTYPES="true")) == BASE + MX + DTYPES + FP + SPARSE
    assert _args("sparse", {"GPU_PROBE_SPARSE": "false"}) == BASE + SPARSE


def test_unknown_token_ignores_the_whole_value():
    for value in ("sparse,bogus", "false,sparse", "sparse,", "sparsity", "smfmac"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


@pytest.mark.parametrize("sparse_on", [False, True])
def test_values_accepted_before_keep_their_args(sparse_on):
    """Every value the earlier steps' tests list, with the arguments they list for it; under
    ``GPU_PROBE_SPARSE=true`` each probed one gains ``--sparse`` at the end."""
    on = {"GPU_PROBE_SPARSE": "true"} if sparse_on else {}

    def check(value, env, want, **kw):
        assert _args(value, dict(env, **on), **kw) == (want + SPARSE if sparse_on and want is not None else want), \
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
    for value in ("mx,bogus", "yes", "mx,", "false,mx", "dtypes,bogus", "false,dtypes", "dtype", "fp,bogus", "fp32"):
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


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_SPARSE=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_SPARSE=false\n" in f.read()


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
    ("--sparse", "bogus"), ("--sparse", "bf16,bogus"), ("--sparse", "f32"), ("--sparse", "fp4"), ("--sparse", ""),
    ("--sparse", "bf16,"), ("--sparse", "i8,i8"), ("--sparse", "bf16,f16,bf16"),
    ("--inject-fault", "sparse"), ("--fp", "f32", "--inject-fault", "sparse"),
    # K = 64 is half a stage of an 8-bit format (and has zero classes); 320 has none and is still no i8 stage
    ("--sparse", "i8", "--shape", "256,256,64"), ("--sparse", "bf16,fp8", "--shape", "256,256,320"),
    # a K at which a class of the pruned operands expects 0
    ("--sparse", "bf16", "--shape", "256,256,64"), ("--sparse", "bf16", "--shape", "256,256,128"),
    ("--sparse", "i8", "--shape", "4096,4096,768"), ("--sparse", "bf16,f16,i8,fp8,bf8", "--shape", "4096,4096,2048")])
def test_program_sparse_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert "[--sparse bf16,f16,i8,fp8,bf8]" in r.stderr and "[--fp f32,f64]" in r.stderr
    assert "rccl|mx|dtypes|fp]" in r.stderr and "[--inject-fault sparse]" in r.stderr


def test_program_no_gpu_verdict_with_sparse():
    r = _run("--sparse", "bf16,f16,i8,fp8,bf8")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "sparse" not in res
    # accepted next to the other steps, in any order, one format alone, and with its fault hook
    assert _run("--mx", "fp8,fp4", "--sparse", "bf8,i8", "--fp", "f64,f32").returncode == probe_main.NO_GPU
    assert _run("--sparse", "fp8,bf16", "--dtypes", "f16,i8", "--mx", "fp8,fp4,bf8,fp6,bf6", "--fp", "f32,f64",
                "--inject-fault", "sparse").returncode == probe_main.NO_GPU
    assert _run("--sparse=i8", "--inject-fault=sparse").returncode == probe_main.NO_GPU
    # K = 320 has no zero class and is five stages of the 16-bit formats; 640 serves all
    assert _run("--sparse", "bf16,f16", "--shape", "256,256,320").returncode == probe_main.NO_GPU
    assert _run("--sparse", "bf16,i8,bf8", "--shape", "256,256,640").returncode == probe_main.NO_GPU
    # without --sparse those K stay as acceptable as they were
    assert _run("--shape", "256,256,128").returncode == probe_main.NO_GPU
    assert _run("--dtypes", "i8", "--shape", "256,256,64").returncode == probe_main.NO_GPU


# ------------------------------------------------------------------ ABI mirror


def test_constants_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        header = dict(re.findall(r"^\s*(ODH_SP_\w+)\s*=\s*(\d+)\s*,", f.read(), re.M))
    assert {k: int(v) for k, v in header.items()} == {
        "ODH_SP_BF16": gpu.ODH_SP_BF16, "ODH_SP_F16": gpu.ODH_SP_F16, "ODH_SP_I8": gpu.ODH_SP_I8,
        "ODH_SP_FP8": gpu.ODH_SP_FP8, "ODH_SP_BF8": gpu.ODH_SP_BF8, "ODH_SP_CLASSES": 210}
    for name, value in header.items():
        assert getattr(gpu, name) == int(value), name
    assert list(gpu.SPARSE_FORMATS) == sp.FORMATS and len(set(gpu.SPARSE_FORMATS.values())) == 5
    assert gpu.SPARSE_TABLE == sp.CLASSES and gpu.SPARSE_TABLE[0] * gpu.SPARSE_TABLE[1] == gpu.ODH_SP_CLASSES
    assert (gpu.ODH_DT_I8_MUL_A, gpu.ODH_DT_I8_MUL_B) == sp.MUL["i8"]
    for name in ("odh_sparse_zero_classes", "odh_sparse_fill", "odh_sparse_gemm", "odh_sparse_probe_gemm_verify"):
        assert name in gpu.SIGNATURES, name
    assert gpu.SIGNATURES["odh_sparse_zero_classes"] == gpu.SIGNATURES["odh_mx_zero_classes"]
    assert len(gpu.SIGNATURES["odh_sparse_fill"][1]) == 9 and len(gpu.SIGNATURES["odh_sparse_gemm"][1]) == 9
    assert len(gpu.SIGNATURES["odh_sparse_probe_gemm_verify"][1]) == 11


def test_sparse_shape_ok_at_the_stage_boundaries():
    assert sp.STAGE == {"bf16": 64, "f16": 64, "i8": 128, "fp8": 128, "bf8": 128}
    for fmt in sp.FORMATS:
        s = sp.STAGE[fmt]
        assert s * sp.ESIZE[fmt] == 128  # 128 bytes of a Bt row
        for k in (s, 2 * s, 64 * s):
            assert gpu.sparse_shape_ok(fmt, 256, 512, k), (fmt, k)
            assert gpu.sparse_shape_ok(gpu.SPARSE_FORMATS[fmt], 256, 512, k), (fmt, k)
        for k in (0, -s, s // 2, s - 1, s + 1, s + s // 2):
            assert not gpu.sparse_shape_ok(fmt, 256, 512, k), (fmt, k)
        for m, n in ((128, 256), (256, 128), (256, 384), (0, 256), (256, 0), (-256, 256)):
            assert not gpu.sparse_shape_ok(fmt, m, n, s), (fmt, m, n)
    assert gpu.sparse_shape_ok("bf16", 256, 256, 64) and not gpu.sparse_shape_ok("i8", 256, 256, 64)
    for bad in ("f32", "fp4", "fp6", 5, -1):
        with pytest.raises(ValueError):
            gpu.sparse_shape_ok(bad, 256, 256, 128)


# ------------------------------------------------------------------ the host model


@pytest.mark.parametrize("k", [128, 256, 1024])
def test_table_is_the_pruned_product(k):
    m, n = 60, 14  # two periods of the classes each way
    a, bt = sp.pruned_operands(m, n, k)
    dense, _ = ref.probe_operands(m, n, k)
    # 2:4, all six pairs in every row, all six nibbles and no other
    assert ((a != 0).reshape(m, k // 4, 4).sum(-1) <= 2).all() and sp.keep_mask(m, k).reshape(m, -1, 4).sum(-1).min() == 2
    nib = sp.nibbles(m, k)
    assert all(set(row.tolist()) == set(sp.VALID_NIBBLES) for row in nib)
    assert all(set(col.tolist()) == set(sp.VALID_NIBBLES) for col in nib.T)
    assert ((nib & 3) < (nib >> 2)).all()
    t = sp.table(k)
    assert t.shape == (30, 7)
    assert np.array_equal(a @ bt.T, t[np.arange(m)[:, None] % 30, np.arange(n)[None, :] % 7])
    for fmt in sp.FORMATS:
        hac, hmeta, hbt = sp.fill(fmt, m, n, k)
        assert np.array_equal(sp.product(hac, hmeta, hbt), sp.expected(fmt, m, n, k))
        assert hac.shape == (m, k // 2) and hmeta.shape == (m, k // 8) and hmeta.dtype == np.uint8
        assert np.array_equal(sp.decompress(hac, hmeta), a * sp.MUL[fmt][0])
        assert not sp.mismatches(fmt, hac, hmeta, hbt, k).any()
    assert sp.zero_classes(k) == {128: 1, 256: 2, 1024: 0}[k]
    if k == 1024:
        assert (t != 0).all() and (t != (dense @ bt.T)[:30, :7]).all()  # no zero class, none equal to the unpruned product
        assert (t.min(), t.max()) == (-40, 41)


def _decoder_passes(k, decode):
    """Classes that a wrong decoder of the metadata would still compute right."""
    m, n = 30, 7
    dense, bt = ref.probe_operands(m, n, k)
    nib = sp.nibbles(m, k)
    ac = sp.compress_with(dense, nib)
    assert np.array_equal(sp.product_per_slot(ac, nib, bt), sp.product(ac, sp.pack_meta(nib), bt))
    return int((sp.product_per_slot(ac, decode(nib), bt) == sp.table(k)).sum())


def test_family_tells_wrong_decoders_apart_at_the_probe_k():
    k = 1024
    swap = lambda nib: (nib >> 2) | ((nib & 3) << 2)  # noqa: E731  the two selectors of a group swapped
    assert _decoder_passes(k, lambda nib: nib) == 210
    assert _decoder_passes(k, swap) == 0
    assert _decoder_passes(k, lambda nib: nib & 0b1010) == 0  # bit 0 of each selector stuck at 0
    assert _decoder_passes(k, lambda nib: nib & 0b0101) == 5  # bit 1 of both selectors stuck at 0: 5 of 210 pass
    assert _decoder_passes(k, lambda nib: nib & 0b0111) == 1  # bit 1 of the second selector alone
    assert _decoder_passes(k, lambda nib: nib & 0b1101) == 6  # bit 1 of the first selector alone
    assert _decoder_passes(k, lambda nib: np.full_like(nib, 4)) == 4  # the index ignored: 4 of 210 pass


def test_zero_classes_agree_with_the_library():
    lib = gpu.load_library()
    for k in range(64, 2049, 64):
        assert lib.odh_sparse_zero_classes(k) == sp.zero_classes(k) == gpu.sparse_zero_classes(k), k
    assert [k for k in range(64, 2049, 64) if sp.zero_classes(k) == 0] == [320, 640, 1024, 1088, 1472, 1856]
    assert (sp.zero_classes(64), sp.zero_classes(128), sp.zero_classes(256)) == (4, 1, 2)
    for k in (0, -64, 32, 100, 1000):
        assert lib.odh_sparse_zero_classes(k) == -1, k


def test_exactness_bound_of_every_format_at_the_probe_shape():
    k = 1024
    a, bt = sp.pruned_operands(30, 7, k)
    for fmt in sp.FORMATS:
        ma, mb = sp.MUL[fmt]
        worst = int((np.abs(a * ma) @ np.abs(bt * mb).T).max())
        assert worst <= 6 * (k // 2) * ma * mb < sp.EXACT_BELOW[fmt], fmt  # |a| <= 2, |b| <= 3, K/2 kept
        assert 2 * ma <= sp.INT_RANGE[fmt] and 3 * mb <= sp.INT_RANGE[fmt], fmt  # the operands are values of the format
    assert 6 * 512 * 25 * 41 == 3148800 < 2 ** 31
    # the codes of the small integers are torch's
    v = np.arange(-3, 4)
    tv = torch.arange(-3, 4).float()
    assert np.array_equal(sp.fp8_code(v), tv.to(torch.float8_e4m3fn).view(torch.uint8).numpy())
    assert np.array_equal(sp.bf8_code(v), tv.to(torch.float8_e5m2).view(torch.uint8).numpy())
    codes = np.arange(0, 0x78, dtype=np.uint8)
    for value, dt in ((sp.fp8_value, torch.float8_e4m3fn), (sp.bf8_value, torch.float8_e5m2)):
        both = np.concatenate((codes, codes | 0x80))
        assert np.array_equal(value(both), torch.from_numpy(both).view(dt).double().numpy())


def test_lane_map_model_is_consistent():
    """The measured map as the model states it: a lane's B elements and A slots tile the instruction's
    k, slot and element of a group meet, and the model's one-instruction product is the plain one."""
    rng = np.random.default_rng(24)
    for fmt in sp.FORMATS:
        slots, elems = 16 // sp.ESIZE[fmt], 32 // sp.ESIZE[fmt]
        for col in (0, 31):
            ks = sorted(sp.lane_b_element(fmt, lane, e) for lane in (col, col + 32) for e in range(elems))
            assert ks == list(range(2 * elems))
        kept = sorted(sp.lane_a_slot(fmt, lane, s) for lane in (5, 37) for s in range(slots))
        assert kept == list(range(2 * slots))
        assert [sp.lane_b_element(fmt, 40, e) for e in (0, elems // 2)] == [elems // 2, 3 * elems // 2]  # chunks 1 and 3
        assert sp.lane_index_bits(fmt, 0, 3) == 6 and sp.lane_index_bits(fmt, 63, slots - 1) == 2 * slots - 2
        assert sp.lane_index_bits(fmt, 0, 0, cbsz=0, abid=1) == (16 if sp.ESIZE[fmt] == 2 else 0)
        assert sp.lane_index_bits(fmt, 0, 0, cbsz=1, abid=1) == 0
        # registers as the kernel loads them from the public layout, one instruction
        kk = 2 * elems
        ac = rng.integers(-3, 4, size=(32, kk // 2))
        nib = rng.choice(sp.VALID_NIBBLES, size=(32, kk // 4))
        bt = rng.integers(-3, 4, size=(32, kk))
        a_regs = np.array([[ac[lane & 31, sp.lane_a_slot(fmt, lane, s)] for s in range(slots)] for lane in range(64)])
        b_regs = np.array([[bt[lane & 31, sp.lane_b_element(fmt, lane, e)] for e in range(elems)] for lane in range(64)])
        idx = np.zeros(64, dtype=np.int64)
        for lane in range(64):
            groups = slots // 2
            for g in range(groups):
                idx[lane] |= int(nib[lane & 31, (lane >> 5) * groups + g]) << (4 * g)
        want = sp.product(ac, sp.pack_meta(nib), bt)
        assert np.array_equal(sp.instruction(fmt, a_regs, b_regs, idx), want), fmt
        ac_, meta_, bt_, want_ = sp.lanemap_case(fmt)
        assert ((ac_ != 0).sum(1) == 1).all() and set(np.unique(sp.unpack_meta(meta_)).tolist()) <= set(sp.VALID_NIBBLES)
        hot = np.argmax(ac_ != 0, axis=1)
        assert set(hot.tolist()) == set(range(sp.STAGE[fmt] // 2))  # every kept slot of a stage


# ------------------------------------------------------------------ sparse_compress / sparse_decompress


DTYPES_T = [torch.bfloat16, torch.float16, torch.int8, torch.float8_e4m3fn, torch.float8_e5m2, torch.float32]


def _as(dtype, ints):
    t = torch.from_numpy(np.asarray(ints))
    return t.to(torch.int8) if dtype == torch.int8 else t.float().to(dtype)


def _np(t):
    return t.numpy().astype(np.int64) if t.dtype == torch.int8 else t.float().numpy().astype(np.int64)


@pytest.mark.parametrize("dtype", DTYPES_T)
def test_compress_round_trip_on_the_family_and_random_data(dtype):
    a, _ = sp.pruned_operands(64, 1, 128)
    ac, meta = gpu.sparse_compress(_as(dtype, a))
    assert ac.dtype == dtype and tuple(ac.shape) == (64, 64) and meta.dtype == torch.uint8 and tuple(meta.shape) == (64, 16)
    hac, hmeta = sp.compress(a)
    assert np.array_equal(_np(ac), hac) and np.array_equal(meta.numpy(), hmeta)
    # where the family keeps two non-zeros the nibble is the selector's
    both = (a != 0).reshape(64, 32, 4).sum(-1) == 2
    assert np.array_equal(sp.unpack_meta(hmeta)[both], sp.nibbles(64, 128)[both])
    assert np.array_equal(_np(gpu.sparse_decompress(ac, meta)), a)
    rng = np.random.default_rng(11)
    r = rng.integers(-7, 8, size=(40, 64))
    r[rng.random(r.shape) < 0.3] = 0
    pac, pmeta = gpu.sparse_compress(_as(dtype, r), prune=True)
    hac, hmeta = sp.compress(r, prune=True)
    assert np.array_equal(_np(pac), hac) and np.array_equal(pmeta.numpy(), hmeta)
    pruned = _np(gpu.sparse_decompress(pac, pmeta))
    assert np.array_equal(pruned, sp.decompress(hac, hmeta))
    # 2:4, and what is kept are the two largest magnitudes of every group
    g, full = np.abs(pruned.reshape(40, 16, 4)), np.abs(r.reshape(40, 16, 4))
    assert ((g != 0).sum(-1) <= 2).all()
    assert np.array_equal(np.sort(g, axis=-1)[..., 2:], np.sort(full, axis=-1)[..., 2:])
    nib = sp.unpack_meta(pmeta.numpy())
    assert ((nib & 3) < (nib >> 2)).all()
    # compressing the pruned matrix without prune is the same pair of tensors
    ac2, meta2 = gpu.sparse_compress(gpu.sparse_decompress(pac, pmeta))
    assert np.array_equal(_np(ac2), _np(pac)) and torch.equal(meta2, pmeta)


def test_compress_refuses_and_prunes():
    with pytest.raises(ValueError, match="row 1, group 2"):
        gpu.sparse_compress(torch.tensor([[0] * 16, [0, 0, 0, 0, 1, 0, 0, 1, 1, 2, 0, 3, 0, 0, 0, 0]]))
    for bad in (torch.zeros(4), torch.zeros((2, 12)), torch.zeros((2, 2, 8))):
        with pytest.raises(ValueError):
            gpu.sparse_compress(bad)
    # ties to the lower position; fewer than two non-zeros still give p0 < p1
    ac, meta = gpu.sparse_compress(torch.tensor([[3, -3, 3, 3, 0, 0, 0, 5]]), prune=True)
    assert ac.tolist() == [[3, -3, 0, 5]] and meta.tolist() == [[0b1100_0100]]
    ac, meta = gpu.sparse_compress(torch.tensor([[1, 5, -7, 2, 0, 9, 0, 0]]), prune=True)
    assert ac.tolist() == [[5, -7, 0, 9]] and meta.tolist() == [[0b0100_1001]]
    ac, meta = gpu.sparse_compress(torch.zeros((1, 8)))
    assert meta.tolist() == [[0x44]] and not ac.any()
    assert gpu.sparse_decompress(*gpu.sparse_compress(torch.tensor([[0, 0, 7, 0, 0, 0, 0, 0]]))).tolist() == \
        [[0, 0, 7, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        gpu.sparse_decompress(torch.zeros((2, 4)), torch.zeros((2, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        gpu.sparse_decompress(torch.zeros((2, 4)), torch.zeros((2, 1), dtype=torch.int8))


# ------------------------------------------------------------------ the models of the sweeps and the value cases


SWEEP = (512, 512, 640)  # the shape of tests/test_gpu_sparse_fp_sweeps.py


@pytest.mark.parametrize("fmt", ["fp8", "bf8"])
def test_code_values_are_torchs_for_every_code(fmt):
    codes = np.arange(256, dtype=np.uint8)
    theirs = torch.from_numpy(codes).view(torch.float8_e4m3fn if fmt == "fp8" else torch.float8_e5m2).double().numpy()
    ours = sp.code_values(fmt)
    assert np.array_equal(np.isnan(ours), np.isnan(theirs)) and np.array_equal(ours[~np.isnan(ours)], theirs[~np.isnan(theirs)])
    assert np.array_equal(np.signbit(ours[~np.isnan(ours)]), np.signbit(theirs[~np.isnan(theirs)]))  # -0 is -0
    if fmt == "fp8":
        assert np.flatnonzero(np.isnan(ours)).tolist() == [0x7F, 0xFF] and not np.isinf(ours).any()
        assert np.nanmax(ours) == 448 and ours[1] == 2.0 ** -9
    else:
        assert np.flatnonzero(np.isnan(ours)).tolist() == [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]
        assert ours[0x7C] == np.inf and ours[0xFC] == -np.inf and ours[0x7B] == 57344 and ours[1] == 2.0 ** -16


@pytest.mark.parametrize("fmt", sp.FORMATS)
def test_stored_elements_round_trip(fmt):
    m, n, k = 30, 7, 128
    hac, hmeta, hbt = sp.fill(fmt, m, n, k)
    for ints in (hac, hbt):
        stored = sp.encode(fmt, ints)
        assert stored.dtype == sp.NP_STORED[fmt] and stored.itemsize == sp.ESIZE[fmt]
        assert np.array_equal(sp.decode(fmt, stored), ints)
        assert not np.signbit(sp.decode(fmt, stored)[ints == 0]).any()  # the fill writes no -0
    if fmt == "bf16":
        t = torch.from_numpy(sp.encode(fmt, hbt)).view(torch.bfloat16)
        assert np.array_equal(t.double().numpy(), hbt)
        bits = np.array([0x7FC0, 0x7F80, 0xFF80, 0x0080, 0x7F7F], dtype=np.uint16).view(np.int16)
        got = sp.decode(fmt, bits)
        assert np.isnan(got[0]) and got[1:].tolist() == [np.inf, -np.inf, 2.0 ** -126, (2 - 2.0 ** -7) * 2.0 ** 127]
    if fmt == "f16":
        assert np.isnan(sp.decode(fmt, np.array([0x7E00], dtype=np.uint16).view(np.float16))[0])


@pytest.mark.parametrize("fmt", sp.FORMATS)
def test_value_sweeps_change_one_element_a_line_and_no_launch_is_vacuous(fmt):
    m, n, k = SWEEP
    hac, hmeta, hbt = sp.fill(fmt, m, n, k)
    expect = sp.expected(fmt, m, n, k)
    assert np.array_equal(sp.product(hac, hmeta, hbt), expect)
    for side, clean in ((0, hac), (1, hbt)):
        wrong = sp.sweep_values(fmt, clean, side)
        x = np.arange(clean.shape[0])
        assert np.array_equal(np.argwhere(wrong != clean), np.stack([x, x % clean.shape[1]], axis=1))
        mul = sp.MUL[fmt][side]
        assert set(np.unique(wrong[x, x % clean.shape[1]] // mul).tolist()) == {1, 2} and not (wrong % mul).any()
        assert np.array_equal(sp.decode(fmt, sp.encode(fmt, wrong)), wrong)  # values of the format
        ops = (wrong, hmeta, hbt) if side == 0 else (hac, hmeta, wrong)
        assert (np.abs(sp.decompress(ops[0], hmeta)) @ np.abs(ops[2]).T).max() < sp.EXACT_BELOW[fmt]
        mismatch = sp.product(*ops) != expect
        lines = mismatch if side == 0 else mismatch.T
        # launch x has element x alone: its line x is line x of this product, every other line is clean
        counts = lines.sum(axis=1)
        assert (counts.min(), counts.max()) == ((438, 439) if side == 0 else (204, 206))
        one = clean.copy()
        one[300, 300 % clean.shape[1]] = wrong[300, 300 % clean.shape[1]]
        alone = sp.product(*((one, hmeta, hbt) if side == 0 else (hac, hmeta, one))) != expect
        alone = alone if side == 0 else alone.T
        assert np.array_equal(alone[300], lines[300]) and not np.delete(alone, 300, axis=0).any()
    # a changed B element is wrong only in the rows that keep its k with a non-zero value
    dense = sp.decompress(hac, hmeta)
    wrong = sp.sweep_values(fmt, hbt, 1)
    mismatch = sp.product(hac, hmeta, wrong) != expect
    for j in (0, 77, 511):
        assert np.array_equal(mismatch[:, j], dense[:, j % k] != 0)
    # the slots of the A sweep are every place of the kernel's operand feed
    stages = k // sp.STAGE[fmt]
    places = set(zip(*(np.asarray(c).tolist() for c in sp.kept_slot_coordinates(fmt, np.arange(m) % (k // 2)))))
    assert len(places) == k // 2 == stages * 2 * 2 * (8 // sp.ESIZE[fmt]) * 2
    assert sp.kept_slot_coordinates("bf16", 319) == (9, 1, 1, 3, 1) and sp.kept_slot_coordinates("i8", 319) == (4, 1, 1, 7, 1)
    assert sp.kept_slot_coordinates("f16", 8) == (0, 0, 1, 0, 0) and sp.kept_slot_coordinates("fp8", 32) == (0, 1, 0, 0, 0)


def test_nibble_plan_covers_every_group_nibble_and_byte_half():
    m, n, k = SWEEP
    group, new, moved = sp.nibble_sweep_plan(m, n, k)
    assert set(group.tolist()) == set(range(k // 4)) and set(new.tolist()) == set(sp.VALID_NIBBLES)
    assert set((group % 2).tolist()) == {0, 1} and 0 < moved < m // 4
    # it starts at group i mod (K/4) and rarely moves to the next group
    assert (((group - np.arange(m)) % (k // 4)) <= 1).all()
    for fmt in sp.FORMATS:
        hac, hmeta, hbt = sp.fill(fmt, m, n, k)
        wrong = sp.meta_with_nibbles(hmeta, group, new)
        assert np.array_equal(np.argwhere(wrong != hmeta), np.stack([np.arange(m), group // 2], axis=1))
        was, now = sp.unpack_meta(hmeta), sp.unpack_meta(wrong)
        assert np.array_equal(np.argwhere(was != now), np.stack([np.arange(m), group], axis=1))  # the one nibble
        mismatch = sp.product(hac, wrong, hbt) != sp.expected(fmt, m, n, k)
        counts = mismatch.sum(axis=1)
        assert counts.min() > 0 and counts.max() <= n, fmt  # no launch is vacuous
        assert np.array_equal(sp.product_per_slot(hac, now, hbt), sp.product(hac, wrong, hbt))
    print("nibble plan:", moved, "rows moved on; mismatches a launch", counts.min(), "..", counts.max())


def test_per_slot_product_in_float64_multiplies_only_what_a_row_keeps():
    m, n, k = 60, 14, 128
    for fmt in ("f16", "bf8"):
        hac, hmeta, hbt = sp.fill(fmt, m, n, k)
        nib = sp.unpack_meta(hmeta)
        clean = sp.product_per_slot_f64(hac, nib, hbt)
        assert clean.dtype == np.float64 and np.array_equal(clean, sp.expected(fmt, m, n, k))
        keep = sp.keep_mask(m, k)
        for bad in (np.nan, np.inf):
            j, kk = 9, 77
            b = hbt.astype(np.float64)
            b[j, kk] = bad
            got = sp.product_per_slot_f64(hac, nib, b)
            assert np.array_equal(np.isnan(got) | np.isinf(got), np.outer(keep[:, kk], np.arange(n) == j))
            kept_zero = keep[:, kk] & (sp.decompress(hac, hmeta)[:, kk] == 0)
            assert kept_zero.any() and np.isnan(got[kept_zero, j]).all()  # 0 · inf and 0 · NaN
            i, slot = 31, 40
            a = hac.astype(np.float64)
            a[i, slot] = bad
            got = sp.product_per_slot_f64(a, nib, hbt)
            assert not np.isfinite(got[i]).any() and np.array_equal(np.delete(got, i, axis=0), np.delete(clean, i, axis=0))


@pytest.mark.parametrize("fmt,swap", [(f, False) for f in sp.FORMATS] + [("bf16", True)])
def test_onehot_case_is_one_exact_product_per_output(fmt, swap):
    ac, meta, bt, want = sp.onehot_case(fmt, swap)
    stage = sp.STAGE[fmt]
    assert ac.shape == (256, stage // 2) and meta.shape == (256, stage // 8) and bt.shape == (256, stage)
    assert ac.dtype == bt.dtype == sp.NP_STORED[fmt] and meta.dtype == np.uint8 and want.shape == (256, 256)
    nib = sp.unpack_meta(meta)
    assert set(np.unique(nib).tolist()) == set(sp.VALID_NIBBLES)
    rows, cols = sp.store_values(fmt, swap)
    i = np.arange(256)
    raw = ac.view(np.uint8).reshape(256, stage // 2, -1).any(axis=2)  # by bits: -0 and NaN are elements too
    hot = i % (stage // 2)
    assert not (raw & (np.arange(stage // 2)[None, :] != hot[:, None])).any()  # +0 everywhere else
    assert np.array_equal(ac[i, hot].view(np.uint8), np.ascontiguousarray(rows).view(np.uint8))
    assert set(hot.tolist()) == set(range(stage // 2))  # every kept slot of the stage
    assert (bt.view(np.uint8).reshape(256, stage, -1) == bt.view(np.uint8).reshape(256, stage, -1)[:, :1]).all()
    va, vb = sp.decode(fmt, rows), sp.decode(fmt, cols)
    if fmt in ("fp8", "bf8", "i8"):  # every pair of codes / values
        assert sorted(np.asarray(rows).view(np.uint8).tolist()) == sorted(np.asarray(cols).view(np.uint8).tolist()) == list(range(256))
    finite = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        single = va[:, None] * vb[None, :]
    # where the model is finite it is the one product, and the same product summed with the row's zeros
    # through the float64 per-slot model, whatever the nibbles select
    assert np.array_equal(want[finite], single[finite])
    full = sp.product_per_slot_f64(sp.decode(fmt, ac), nib, sp.decode(fmt, bt))
    assert np.array_equal(np.isnan(full), np.isnan(want)) and np.array_equal(full[~np.isnan(want)], want[~np.isnan(want)])
    # exact in the accumulator: fp32 holds every finite product (int32 every i8 one)
    if fmt == "i8":
        assert finite.all() and np.abs(want).max() == 128 * 128
    else:
        assert np.array_equal(want[finite].astype(np.float32).astype(np.float64), want[finite])
        nz = finite & (want != 0)
        assert np.abs(want[nz]).min() >= 2.0 ** -126  # normal fp32 numbers
    if fmt == "fp8":
        assert np.isnan(want).sum() == 2 * 256 + 2 * 254 and not np.isinf(want).any()
        assert want[0x7E, 0x7E] == 448.0 * 448.0 and want[1, 1] == 2.0 ** -18
    if fmt == "bf8":
        assert np.isnan(want[:, [0x7C, 0xFC, 0x7D, 0xFF]]).all()  # an infinite or NaN column value: 0 · inf
        assert want[0x7C, 0x3C] == np.inf and want[0x7C, 0xBC] == -np.inf and np.isnan(want[0x7C, 0]) and np.isnan(want[0x7E, 0x3C])
        assert want[0x7B, 0x7B] == 57344.0 ** 2 and want[1, 1] == 2.0 ** -32
    if fmt in ("f16", "bf16"):
        assert finite.all()
    if fmt == "bf16":
        big, small = (sp.decode("bf16", x.view(np.int16)) for x in sp.bf16_value_sets())
        assert np.array_equal(va, small if swap else big) and np.array_equal(vb, big if swap else small)
        assert set(range(-8, 9)) <= set(big.tolist()) and {(2 - 2.0 ** -7) * 2.0 ** 127, -(2 - 2.0 ** -7) * 2.0 ** 127} <= set(big.tolist())
        assert 2.0 ** -126 in small.tolist() and np.signbit(big[big == 0]).any() and np.signbit(small[small == 0]).any()
        assert np.abs(big[big != 0]).min() >= 1 and np.abs(small[small != 0]).max() < 0.5 and np.abs(small[small != 0]).min() == 2.0 ** -126
        ones = lambda v: (v.view(np.uint16) & 0x7F) == 0x7F  # noqa: E731
        assert ones(sp.bf16_value_sets()[0]).sum() >= 127 and ones(sp.bf16_value_sets()[1]).sum() >= 125
    if fmt == "f16":
        assert np.array_equal(want, ref.f16_onehot_case()[2])
