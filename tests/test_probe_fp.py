"""The FP32 / FP64 step of the start-up probe, without a GPU.

* the controller: the ``fp`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_FP``, with every value
  accepted before producing the arguments it produced;
* ``odh-gpu-probe --fp``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants against ``gpu_probe.h``;
* the host model (``fp_reference.py``): the scaled 5 × 7 closed form against the full product of
  the operands as the fill encodes them, the exactness bound, and the one-hot cases.
"""

from __future__ import annotations

import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fp_reference as fp
import probe_reference as ref
from odh_kubeflow_amd.controllers import notebook as nbc
from odh_kubeflow_amd.controllers.notebook import (GPU_PROBE_ANNOTATION, GPU_PROBE_CONTAINER, generate_statefulset)
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.ops import gpu, probe_main

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


def test_fp_token_adds_the_step_after_the_others():
    assert nbc.GPU_PROBE_FP_FORMATS == "f32,f64" and nbc.GPU_PROBE_MORE_TOKENS == ("fp",)
    assert "fp" not in nbc.GPU_PROBE_TOKENS
    assert _args("fp") == BASE + FP
    assert _args("fp", gpus=1) == BASE + FP
    assert _args("true,fp") == BASE + FP
    assert _args("rccl,mxall,dtypes,fp") == BASE + RCCL + MX_ALL + DTYPES + FP
    assert _args(" FP , dtypes,rccl ") == BASE + RCCL + DTYPES + FP
    # with every subset of the other tokens, in either order of the list
    others = {"rccl": RCCL, "mx": MX, "mxall": MX_ALL, "dtypes": DTYPES}
    for r in range(len(others) + 1):
        for subset in itertools.combinations(others, r):
            want = list(BASE)
            for token in ("rccl", "mxall" if "mxall" in subset else "mx", "dtypes"):
                if token in subset:
                    want += others[token]
            assert _args(",".join(subset + ("fp",))) == want + FP, subset
            assert _args(",".join(("fp",) + subset)) == want + FP, subset
            if subset:
                assert _args(",".join(subset)) == want, subset  # and without it, what it was


def test_operator_switch_adds_fp_to_every_probed_notebook():
    on = {"GPU_PROBE_FP": "true"}
    assert _args("true", on) == BASE + FP
    assert _args("rccl", on) == BASE + RCCL + FP
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + FP
    assert _args(None, on) is None  # it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("mx", dict(on, GPU_PROBE_MX="true", GPU_PROBE_DTYPES="true")) == BASE + MX + DTYPES + FP
    assert _args("fp", {"GPU_PROBE_FP": "false"}) == BASE + FP


def test_unknown_token_ignores_the_whole_value():
    for value in ("fp,bogus", "false,fp", "fp,", "fp32"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


@pytest.mark.parametrize("fp_on", [False, True])
def test_values_accepted_before_keep_their_args(fp_on):
    """Every value ``test_probe_mx.py`` and ``test_probe_dtypes.py`` list, with the arguments they
    list for it; under ``GPU_PROBE_FP=true`` each probed one gains ``--fp`` at the end."""
    on = {"GPU_PROBE_FP": "true"} if fp_on else {}

    def check(value, env, want, **kw):
        assert _args(value, dict(env, **on), **kw) == (want + FP if fp_on and want is not None else want), (value, env)

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
    check("rccl", mx_on, BASE + RCCL + MX)
    check(None, dict(mx_on, **startup), BASE + MX)
    check(None, mx_on, None)
    check("false", dict(mx_on, **startup), None)
    for value in ("mx,bogus", "yes", "mx,", "false,mx", "dtypes,bogus", "dtypes,", "false,dtypes", "dtype"):
        check(value, {}, None)
        check(value, startup, BASE)
    check("dtypes", {}, BASE + DTYPES)
    check("rccl,mx,dtypes", {}, BASE + RCCL + MX + DTYPES)
    check(" DTYPES , mx,rccl ", {}, BASE + RCCL + MX + DTYPES)
    check("true,dtypes", {}, BASE + DTYPES)
    check("dtypes", {}, BASE + DTYPES, gpus=1)
    check("mx,dtypes", {}, BASE + MX + DTYPES)
    check("mxall", {}, BASE + MX_ALL)
    check("mx,mxall,dtypes", {}, BASE + MX_ALL + DTYPES)
    dt_on = {"GPU_PROBE_DTYPES": "true"}
    check("true", dt_on, BASE + DTYPES)
    check("rccl", dt_on, BASE + RCCL + DTYPES)
    check(None, dict(dt_on, **startup), BASE + DTYPES)
    check(None, dt_on, None)
    check("false", dict(dt_on, **startup), None)
    check("mx", dict(dt_on, **mx_on), BASE + MX + DTYPES)
    check("true", {"GPU_PROBE_MX_ALL": "true"}, BASE + MX_ALL)
    check("true", {"GPU_PROBE_RCCL": "true"}, BASE + RCCL)
    check("true", {"GPU_PROBE_RCCL": "true"}, BASE, gpus=1)


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_FP=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_FP=false\n" in f.read()


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
    ("--fp", "bogus"), ("--fp", "f32,bogus"), ("--fp", "f16"), ("--fp", ""), ("--fp", "f32,"), ("--fp", "f64,f64"),
    ("--inject-fault", "fp"), ("--dtypes", "f16,i8", "--inject-fault", "fp"),
    # K beyond the exactness bound of a format that is asked for: 2728 (f32), 1365 (f64)
    ("--fp", "f32,f64", "--shape", "4096,4096,1408"), ("--fp", "f64", "--shape", "256,256,1408"),
    ("--fp", "f32", "--shape", "256,256,2752")])
def test_program_fp_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert "[--fp f32,f64]" in r.stderr and "--dtypes f16,i8" in r.stderr and "bf8,fp6,bf6" in r.stderr
    assert "rccl|mx|dtypes|fp]" in r.stderr


def test_program_no_gpu_verdict_with_fp():
    r = _run("--fp", "f32,f64")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "fp" not in res
    # accepted next to the other steps, in either order, one format alone, and with its fault hook
    assert _run("--mx", "fp8,fp4", "--dtypes", "i8,f16", "--fp", "f64,f32").returncode == probe_main.NO_GPU
    assert _run("--fp", "f32,f64", "--dtypes", "f16,i8", "--mx", "fp8,fp4,bf8,fp6,bf6",
                "--inject-fault", "fp").returncode == probe_main.NO_GPU
    assert _run("--fp=f64", "--inject-fault=fp").returncode == probe_main.NO_GPU
    # a K within f32's bound and beyond f64's is fine while f64 is not asked for
    assert _run("--fp", "f32", "--shape", "256,256,1408").returncode == probe_main.NO_GPU


# ------------------------------------------------------------------ ABI mirror


def test_constants_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        header = dict(re.findall(r"^\s*(ODH_FP_\w+)\s*=\s*(\d+)\s*,", f.read(), re.M))
    assert {k: int(v) for k, v in header.items()} == {
        "ODH_FP_F32": gpu.ODH_FP_F32, "ODH_FP_F64": gpu.ODH_FP_F64,
        "ODH_FP_F32_MUL_A": 25, "ODH_FP_F32_MUL_B": 41, "ODH_FP_F64_MUL_A": 1048573, "ODH_FP_F64_MUL_B": 1048575}
    for name, value in header.items():
        assert getattr(gpu, name) == int(value), name
    assert gpu.FP_FORMATS == {"f32": gpu.ODH_FP_F32, "f64": gpu.ODH_FP_F64} and gpu.ODH_FP_F32 != gpu.ODH_FP_F64
    assert (gpu.ODH_FP_F32_MUL_A, gpu.ODH_FP_F32_MUL_B) == fp.MUL["f32"]
    assert (gpu.ODH_FP_F64_MUL_A, gpu.ODH_FP_F64_MUL_B) == fp.MUL["f64"]
    assert gpu.DENSE_FORMATS == {"f16": gpu.ODH_DT_F16, "i8": gpu.ODH_DT_I8}
    for name in ("odh_fp_tiles", "odh_fp_fill", "odh_fp_gemm", "odh_fp_probe_gemm_verify"):
        assert name in gpu.SIGNATURES, name
    for dense, ours in (("odh_dense_fill", "odh_fp_fill"), ("odh_dense_gemm", "odh_fp_gemm"),
                        ("odh_dense_probe_gemm_verify", "odh_fp_probe_gemm_verify")):
        assert gpu.SIGNATURES[ours] == gpu.SIGNATURES[dense]


def test_fp_shape_ok_at_the_stage_boundaries():
    assert fp.STAGE == {"f32": 16, "f64": 8}
    for fmt in fp.FORMATS:
        s = fp.STAGE[fmt]
        for k in (s, 2 * s, 64 * s):
            assert gpu.fp_shape_ok(fmt, 256, 512, k), (fmt, k)
            assert gpu.fp_shape_ok(gpu.FP_FORMATS[fmt], 256, 512, k), (fmt, k)
        for k in (0, -s, s // 2, s - 1, s + 1, s + s // 2):
            assert not gpu.fp_shape_ok(fmt, 256, 512, k), (fmt, k)
        for m, n in ((128, 256), (256, 128), (256, 384), (0, 256), (256, 0), (-256, 256)):
            assert not gpu.fp_shape_ok(fmt, m, n, s), (fmt, m, n)
    assert gpu.fp_shape_ok("f64", 256, 256, 8) and not gpu.fp_shape_ok("f32", 256, 256, 8)
    for bad in ("f16", "bf16", 0, 1, 2):
        with pytest.raises(ValueError):
            gpu.fp_shape_ok(bad, 256, 256, 64)
    assert gpu.fp_k_exact("f32", 2728) and not gpu.fp_k_exact("f32", 2729)
    assert gpu.fp_k_exact("f64", 1365) and not gpu.fp_k_exact("f64", 1366)


# ------------------------------------------------------------------ the host model


@pytest.mark.parametrize("k", [64, 192, 1024])
@pytest.mark.parametrize("fmt", fp.FORMATS)
def test_table_is_the_product_of_the_operands(fmt, k):
    m, n = 15, 21  # three periods of the classes each way
    a, bt = fp.operands(fmt, m, n, k)
    va, vb = fp.operand_values(fmt, m, n, k)
    assert a.dtype == bt.dtype == fp.NP_DTYPE[fmt]
    # the floats are the integers, exactly
    assert np.array_equal(a.astype(np.int64), va) and np.array_equal(bt.astype(np.int64), vb)
    ma, mb = fp.MUL[fmt]
    assert ma % 2 == 1 and mb % 2 == 1
    assert (va.min(), va.max()) == (-2 * ma, 2 * ma) and (vb.min(), vb.max()) == (-3 * mb, 3 * mb)
    want = va @ vb.T
    t = fp.table(fmt, k)
    assert t.shape == (5, 7) and np.array_equal(t, ma * mb * ref.probe_class_table(k))
    assert np.array_equal(want, fp.expected(fmt, m, n, k))
    # at the probe's K no class expects 0, where an all-zero product would pass; the family has two
    # such classes of 35 at K = 64 and at K = 192, as the bf16 probe's own table does
    assert (t != 0).all() if k == 1024 else (t == 0).sum() == ref.zero_classes(k) == 2
    # the exactness bound: every partial sum, in any order, is an integer the accumulator holds
    assert fp.k_exact(fmt, k) and 6 * k * ma * mb < fp.EXACT_BELOW[fmt]
    assert (np.abs(va) @ np.abs(vb).T).max() <= 6 * k * ma * mb
    assert np.array_equal(t.astype(fp.NP_DTYPE[fmt]).astype(np.int64), t)
    # and the same product computed in the format itself is that table
    assert np.array_equal(a @ bt.T, fp.expected(fmt, m, n, k).astype(fp.NP_DTYPE[fmt]))


def test_exactness_bound_at_the_probe_shape():
    assert 6 * 1024 * 25 * 41 == 6297600 < 2 ** 24
    assert 6 * 1024 * 1048573 * 1048575 < 2 ** 53
    assert fp.k_exact("f32", 2728) and not fp.k_exact("f32", 2729)
    assert fp.k_exact("f64", 1365) and not fp.k_exact("f64", 1366)


@pytest.mark.parametrize("fmt", fp.FORMATS)
def test_onehot_case_is_one_rounded_product_per_output(fmt):
    dt, bits_t, mb = fp.NP_DTYPE[fmt], fp.NP_BITS[fmt], fp.MANTISSA[fmt]
    stage = fp.STAGE[fmt]
    a, bt, want = fp.onehot_case(fmt)
    assert a.dtype == bt.dtype == want.dtype == dt and a.shape == bt.shape == (256, stage) and want.shape == (256, 256)
    i = np.arange(256)
    va, vb = a[i, i % stage], bt[:, 0]
    assert ((a != 0).sum(axis=1) == 1).all() and (bt == vb[:, None]).all()
    tiny, huge = np.finfo(dt).tiny, np.finfo(dt).max
    for v in (va, vb):
        mant = v.view(bits_t).astype(np.int64) & ((1 << mb) - 1)
        assert np.isfinite(v).all() and (np.abs(v) >= tiny).all()  # normal numbers
        assert ((mant == (1 << mb) - 1).sum() >= 64)  # all-ones mantissas
        single = mant[(mant != 0) & (mant & (mant - 1) == 0)]
        assert len(set(single.tolist())) >= min(mb, 64)  # every (f32) or 64 (f64) single-bit mantissas
        assert ((mant & (mant - 1)) != 0).sum() >= 100  # full mantissas
        e = np.frexp(v.astype(np.float64))[1]
        assert e.max() - e.min() >= (120 if fmt == "f32" else 1000) and (v < 0).any() and (v > 0).any()
    # every product is a normal number, and it is the one RNE rounding of the exact product
    assert np.isfinite(want).all() and (np.abs(want) >= tiny).all() and (np.abs(want) <= huge).all()
    if fmt == "f32":
        exact = va.astype(np.float64)[:, None] * vb.astype(np.float64)[None, :]  # 48 bits: exact in float64
        assert np.array_equal(want, exact.astype(np.float32))
        assert (want.astype(np.float64) != exact).mean() > 0.5  # most of them do round
    else:
        from fractions import Fraction
        for x, y in ((0, 0), (1, 2), (17, 200), (255, 255), (128, 3)):
            exact = Fraction(float(va[x])) * Fraction(float(vb[y]))
            got = Fraction(float(want[x, y]))
            ulp = Fraction(float(np.spacing(np.abs(want[x, y]))))
            assert abs(got - exact) * 2 <= ulp, (x, y)
    assert np.array_equal(want, va[:, None] * vb[None, :])


@pytest.mark.parametrize("fmt", fp.FORMATS)
def test_swept_operands_stay_exact_and_no_launch_is_vacuous(fmt):
    """The operands of the GPU sweeps (``test_gpu_sparse_fp_sweeps.py``): 512 × 512 at 7 stages."""
    m = n = 512
    k = 7 * fp.STAGE[fmt]
    assert k == {"f32": 112, "f64": 56}[fmt] and k % 35 != 0 and fp.k_exact(fmt, k) and gpu.fp_k_exact(fmt, k)
    assert k // fp.STAGE[fmt] > 4  # more stages than ring slots
    assert fp.tiles(fmt, m, n) == {"f32": 4, "f64": 8}[fmt] and n // fp.TILE_N[fmt] == {"f32": 2, "f64": 4}[fmt]
    va, vb = fp.operand_values(fmt, m, n, k)
    expect = fp.expected(fmt, m, n, k)
    assert np.array_equal(va @ vb.T, expect)
    for side, clean, other in ((0, va, vb), (1, vb, va)):
        wrong = fp.sweep_values(fmt, clean, side)
        x = np.arange(512)
        assert np.array_equal(np.argwhere(wrong != clean), np.stack([x, x % k], axis=1))
        assert np.array_equal((wrong - clean)[x, x % k], np.full(512, fp.MUL[fmt][side]))
        # exact: with every changed element at once the sums of magnitudes stay below the accumulator's
        # integer range, and the floats are the integers
        assert (np.abs(wrong) @ np.abs(other).T).max() < fp.EXACT_BELOW[fmt]
        assert np.array_equal(wrong.astype(fp.NP_DTYPE[fmt]).astype(np.int64), wrong)
        mismatch = (wrong @ vb.T if side == 0 else va @ wrong.T) != expect
        counts = (mismatch if side == 0 else mismatch.T).sum(axis=1)
        assert set(counts.tolist()) == ({438, 439} if side == 0 else {409, 410})
