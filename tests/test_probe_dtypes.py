"""The FP16 / INT8 step of the start-up probe, without a GPU.

* the controller: the ``dtypes`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_DTYPES``, with
  every value accepted before producing the arguments it produced;
* ``odh-gpu-probe --dtypes``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants against ``gpu_probe.h``;
* the host model: the bf16 probe's 5 × 7 closed form (``probe_reference.py``) against the full
  product of the operands as the f16 and i8 fills encode them.
"""

from __future__ import annotations

import json
import os
import re
import subprocess

import numpy as np
import pytest

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
DTYPES = ["--dtypes", "f16,i8"]


def test_dtypes_token_adds_the_step_after_the_others():
    assert nbc.GPU_PROBE_DTYPES_FORMATS == "f16,i8" and "dtypes" in nbc.GPU_PROBE_TOKENS
    assert _args("dtypes") == BASE + DTYPES
    assert _args("rccl,mx,dtypes") == BASE + RCCL + MX + DTYPES
    assert _args(" DTYPES , mx,rccl ") == _args("rccl,mx,dtypes")
    assert _args("true,dtypes") == _args("dtypes")
    assert _args("dtypes", gpus=1) == BASE + DTYPES
    assert _args("mx,dtypes") == BASE + MX + DTYPES


def test_operator_switch_adds_dtypes_to_every_probed_notebook():
    on = {"GPU_PROBE_DTYPES": "true"}
    assert _args("true", on) == BASE + DTYPES
    assert _args("rccl", on) == BASE + RCCL + DTYPES
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + DTYPES
    assert _args(None, on) is None  # it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("mx", dict(on, GPU_PROBE_MX="true")) == BASE + MX + DTYPES


def test_unknown_token_ignores_the_whole_value():
    for value in ("dtypes,bogus", "dtypes,", "false,dtypes", "dtype"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


def test_values_accepted_before_keep_their_args():
    """Every value ``test_probe_mx.py`` lists, with the arguments it lists for it."""
    assert _args("true") == BASE
    assert _args("rccl") == BASE + RCCL
    assert _args("false", {"GPU_STARTUP_PROBE": "true"}) is None
    assert _args(None) is None and _args(None, {"GPU_STARTUP_PROBE": "true"}) == BASE
    assert _args("mx") == BASE + MX
    assert _args("rccl,mx") == BASE + RCCL + MX
    assert _args(" MX , rccl ") == BASE + RCCL + MX
    assert _args("true,mx") == BASE + MX
    assert _args("mx", gpus=1) == BASE + MX
    mx_on = {"GPU_PROBE_MX": "true"}
    assert _args("true", mx_on) == BASE + MX
    assert _args("rccl", mx_on) == BASE + RCCL + MX
    assert _args(None, dict(mx_on, GPU_STARTUP_PROBE="true")) == BASE + MX
    assert _args(None, mx_on) is None
    assert _args("false", dict(mx_on, GPU_STARTUP_PROBE="true")) is None
    for value in ("mx,bogus", "yes", "mx,", "false,mx"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_DTYPES=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_DTYPES=false\n" in f.read()


# ------------------------------------------------------------------ the program


def _exe():
    path = probe_main.executable()
    if not os.path.exists(path):
        pytest.fail("odh-gpu-probe not built: python -m odh_kubeflow_amd.ops.build")
    return path


def _run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # a pod without GPUs (also on a GPU machine)
    return subprocess.run([_exe(), "--json", "-", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args", [("--dtypes", "bogus"), ("--dtypes", "f16,bogus"), ("--dtypes", ""),
                                  ("--dtypes", "i8,i8"), ("--inject-fault", "dtypes")])
def test_program_dtypes_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert "--dtypes f16,i8" in r.stderr


def test_program_no_gpu_verdict_with_dtypes():
    r = _run("--dtypes", "f16,i8")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "dtypes" not in res
    # accepted next to the other steps, in either order of the list, and with its fault hook
    assert _run("--mx", "fp8,fp4", "--dtypes", "i8,f16", "--inject-fault", "dtypes").returncode == probe_main.NO_GPU


# ------------------------------------------------------------------ ABI mirror


def test_constants_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        header = dict(re.findall(r"\b(ODH_DT_\w+)\s*=\s*(\d+)\s*,", f.read()))
    assert {k: int(v) for k, v in header.items()} == {
        "ODH_DT_F16": 1, "ODH_DT_I8": 2, "ODH_DT_I8_MUL_A": 25, "ODH_DT_I8_MUL_B": 41}
    for name, value in header.items():
        assert getattr(gpu, name) == int(value), name
    assert gpu.DENSE_FORMATS == {"f16": gpu.ODH_DT_F16, "i8": gpu.ODH_DT_I8}
    assert gpu.MX_FORMATS == {"fp8": 0, "fp4": 4}
    for name in ("odh_dense_fill", "odh_dense_gemm", "odh_dense_probe_gemm_verify"):
        assert name in gpu.SIGNATURES, name
    assert gpu.dense_shape_ok("f16", 256, 512, 32) and not gpu.dense_shape_ok("i8", 256, 512, 32)
    assert gpu.dense_shape_ok("i8", 256, 512, 64) and not gpu.dense_shape_ok("f16", 128, 512, 64)
    with pytest.raises(ValueError):
        gpu.dense_shape_ok("bf16", 256, 256, 64)


# ------------------------------------------------------------------ the host model


def dense_operands(fmt, m, n, k):
    """The operands as ``dense_fill_kernel`` encodes them: the probe's families as halves, or as
    int8 times 25 (A) and 41 (Bt)."""
    a, bt = ref.probe_operands(m, n, k)
    if fmt == "i8":
        a, bt = a * gpu.ODH_DT_I8_MUL_A, bt * gpu.ODH_DT_I8_MUL_B
        assert np.abs(a).max() <= 127 and np.abs(bt).max() <= 127
        return a.astype(np.int8), bt.astype(np.int8)
    return a.astype(np.float16), bt.astype(np.float16)


def dense_table(fmt, k):
    """Expected ``C[i][j]`` by ``(i mod 5, j mod 7)``: the bf16 probe's table, times 1025 for i8."""
    return ref.probe_class_table(k) * (gpu.ODH_DT_I8_MUL_A * gpu.ODH_DT_I8_MUL_B if fmt == "i8" else 1)


@pytest.mark.parametrize("k", [64, 192, 1024])
@pytest.mark.parametrize("fmt", ["f16", "i8"])
def test_table_is_the_product_of_the_operands(fmt, k):
    m, n = 15, 21  # three periods of the classes each way
    a, bt = dense_operands(fmt, m, n, k)
    if fmt == "i8":
        assert a.dtype == np.int8 and (a.min(), a.max()) == (-50, 50)
        assert bt.dtype == np.int8 and (bt.min(), bt.max()) == (-123, 123)
        assert gpu.ODH_DT_I8_MUL_A * gpu.ODH_DT_I8_MUL_B == 1025
        assert 1025 * 6 * k < 2 ** 31  # the bound of gpu_probe_dense.h: exact in int32
    else:
        assert a.dtype == np.float16 and np.array_equal(a.astype(np.int64), ref.probe_operands(m, n, k)[0])
    want = a.astype(np.int64) @ bt.astype(np.int64).T
    t = dense_table(fmt, k)
    assert np.array_equal(want, t[np.arange(m)[:, None] % 5, np.arange(n)[None, :] % 7])
    assert t.any()  # K % 35 != 0: not the vacuous all-zero check


def test_f16_onehot_case_is_exact_in_fp32():
    v = ref.f16_values()
    assert v.dtype == np.uint16 and v.size == 256
    e = (v >> 10) & 31
    assert (((e >= 1) & (e <= 30)) | ((v & 0x7FFF) == 0)).all()  # normal or ±0: no subnormal, inf, NaN
    x = v.view(np.float16).astype(np.float64)
    for want in (*range(-8, 9), 65504.0, -65504.0, 2.0 ** -14):
        assert want in x
    assert {0x0000, 0x8000} <= set(v.tolist())
    assert all(((ee << 10) | 0x3FF) in v for ee in range(1, 31))  # all-ones mantissas
    a, bt, want = ref.f16_onehot_case()
    assert a.dtype == bt.dtype == np.float16 and a.shape == bt.shape == (256, 32)
    nz = (a.view(np.uint16) != 0).sum(axis=1)
    assert np.array_equal(nz, (v != 0).astype(np.int64))  # one non-zero code per row (none for +0)
    assert np.array_equal(a.view(np.uint16)[np.arange(256), np.arange(256) % 32], v)
    assert (bt.view(np.uint16) == v[:, None]).all()
    assert np.isfinite(want).all()
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    nzw = np.abs(want[want != 0])
    assert nzw.min() >= 2.0 ** -28 and nzw.max() <= 65504.0 ** 2  # fp32 normals
    assert np.array_equal(a.astype(np.float64) @ bt.astype(np.float64).T, want)
