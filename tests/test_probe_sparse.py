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
