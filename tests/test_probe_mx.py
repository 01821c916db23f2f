"""The FP8 / MXFP4 step of the start-up probe, without a GPU.

* the controller: ``amd.com/gpu-probe`` as a comma list (``true``, ``rccl``, ``mx``, ``false``) and
  ``GPU_PROBE_MX``, with the values accepted before meaning what they meant;
* ``odh-gpu-probe --mx``: its usage errors and the no-GPU verdict;
* ``odh_mx_zero_classes`` (host arithmetic in the library, through ctypes) against the numpy
  model of ``mx_reference.py``;
* the model itself: the decoder on known FP8 and FP4 codes, and the closed-form table against the full
  product of the decoded, scaled operands.
"""

from __future__ import annotations

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mx_reference as ref
from odh_kubeflow_amd.controllers.notebook import (GPU_PROBE_ANNOTATION, GPU_PROBE_CONTAINER, generate_statefulset)
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.ops import gpu, probe_main
from odh_kubeflow_amd.ops.build import lib_path

# ------------------------------------------------------------------ controller


def _args(value=None, env=None, gpus=2):
    nb = notebook("nb", "ns", gpus=gpus, annotations={GPU_PROBE_ANNOTATION: value} if value is not None else None)
    inits = generate_statefulset(nb, False, env or {})["spec"]["template"]["spec"].get("initContainers") or []
    assert [c["name"] for c in inits] in ([], [GPU_PROBE_CONTAINER])
    return inits[0]["args"] if inits else None


BASE = ["--json", "/dev/termination-log", "--timeout-ms", "30000"]


def test_values_accepted_before_keep_their_args():
    assert _args("true") == BASE
    assert _args("rccl") == BASE + ["--rccl-mib", "64"]
    assert _args("false", {"GPU_STARTUP_PROBE": "true"}) is None
    assert _args(None) is None and _args(None, {"GPU_STARTUP_PROBE": "true"}) == BASE


def test_mx_token_adds_the_mx_step():
    assert _args("mx") == BASE + ["--mx", "fp8,fp4"]
    assert _args("rccl,mx") == BASE + ["--rccl-mib", "64", "--mx", "fp8,fp4"]
    assert _args(" MX , rccl ") == _args("rccl,mx")
    assert _args("true,mx") == _args("mx")
    assert _args("mx", gpus=1) == BASE + ["--mx", "fp8,fp4"]


def test_operator_switch_adds_mx_to_every_probed_notebook():
    assert _args("true", {"GPU_PROBE_MX": "true"}) == BASE + ["--mx", "fp8,fp4"]
    assert _args("rccl", {"GPU_PROBE_MX": "true"}) == BASE + ["--rccl-mib", "64", "--mx", "fp8,fp4"]
    assert _args(None, {"GPU_STARTUP_PROBE": "true", "GPU_PROBE_MX": "true"}) == BASE + ["--mx", "fp8,fp4"]
    assert _args(None, {"GPU_PROBE_MX": "true"}) is None  # it does not turn the probe on
    assert _args("false", {"GPU_STARTUP_PROBE": "true", "GPU_PROBE_MX": "true"}) is None


def test_unknown_token_ignores_the_whole_value():
    for value in ("mx,bogus", "yes", "mx,", "false,mx"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_MX=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_MX=false\n" in f.read()


# ------------------------------------------------------------------ the program


def _exe():
    path = probe_main.executable()
    if not os.path.exists(path):
        pytest.fail("odh-gpu-probe not built: python -m odh_kubeflow_amd.ops.build")
    return path


def _run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # a pod without GPUs (also on a GPU machine)
    return subprocess.run([_exe(), "--json", "-", *args], capture_output=True, text=True, env=env, timeout=60)


def test_program_mx_usage_errors():
    for args in (("--mx", "bogus"), ("--mx", "fp8,bogus"), ("--mx", ""), ("--mx", "fp8,fp8"),
                 ("--mx", "fp4", "--shape", "256,256,192"),  # K is no multiple of 128
                 ("--mx", "fp8", "--shape", "256,256,192"),
                 ("--mx", "fp8", "--shape", "256,256,512"),  # two classes expect 0 at K = 512
                 ("--inject-fault", "mx")):                  # nothing to inject into
        r = _run(*args)
        assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert ref.zero_classes(512) == 2 and ref.zero_classes(384) == 0
    # K = 384 has no such class: a shape like any other, so the verdict is "no GPU", not usage
    assert _run("--mx", "fp8", "--shape", "256,256,384").returncode == probe_main.NO_GPU
    assert _run("--shape", "256,256,192").returncode == probe_main.NO_GPU  # without --mx K = 192 stays legal


def test_program_no_gpu_verdict_with_mx():
    r = _run("--mx", "fp8,fp4")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "mx" not in res


# ------------------------------------------------------------------ odh_mx_zero_classes


def test_zero_classes_match_the_model():
    lib = gpu.bind(ctypes.CDLL(lib_path(probe_main.PROBE_LIB)), ["odh_mx_zero_classes"])
    for k in range(128, 4097, 128):
        assert lib.odh_mx_zero_classes(k) == ref.zero_classes(k), k
    assert [ref.zero_classes(k) for k in (256, 384, 1024, 2048)] == [0, 0, 0, 0]
    assert ref.zero_classes(128) == 12
    for k in (0, -128, 64, 192, 1000):
        assert lib.odh_mx_zero_classes(k) == -1, k


def test_format_constants():
    assert (gpu.ODH_MX_FP8, gpu.ODH_MX_FP4) == (ref.FP8, ref.FP4) == (0, 4)
    assert gpu.MX_FORMATS == {name: ref.NAMES[name] for name in ("fp8", "fp4")} and gpu.MX_ALL_FORMATS == ref.NAMES
    assert gpu.MX_TABLE == (ref.ROWS, ref.COLS)


# ------------------------------------------------------------------ the model


def test_decoders_on_known_codes():
    assert ref.decode_codes(ref.FP8, [0x00, 0x38, 0x40, 0x44, 0xC4, 0x7E, 0x01, 0x08]).tolist() == \
        [0.0, 1.0, 2.0, 3.0, -3.0, 448.0, 2.0 ** -9, 2.0 ** -6]
    assert np.isnan(ref.decode_codes(ref.FP8, [0x7F, 0xFF])).all()
    assert ref.decode(ref.FP4, [0x05, 0x21, 0xF7]).tolist() == [3.0, 0.0, 0.5, 1.0, 6.0, -6.0]
    assert ref.scale_values([126, 127, 130]).tolist() == [0.5, 1.0, 8.0]
    fp4 = np.concatenate([-ref.FP4_VALUES[:0:-1], ref.FP4_VALUES])
    for fmt, vals in ((ref.FP8, np.arange(-8.0, 9.0)), (ref.FP4, fp4)):
        v = np.resize(vals, (2, 64))
        assert np.array_equal(ref.decode(fmt, ref.encode(fmt, v)), v)


@pytest.mark.parametrize("k", [128, 384, 1024])
def test_table_is_the_product_of_the_operands(k):
    m, n = 45, 63  # three periods of the classes each way
    va, vb = ref.probe_values(m, n, k)
    t = ref.probe_table(k)
    for fmt in (ref.FP8, ref.FP4):
        want = ref.product(fmt, ref.encode(fmt, va), ref.encode(fmt, vb), ref.probe_scales(m, k),
                           ref.probe_scales(n, k))
        assert np.array_equal(want, t[np.arange(m)[:, None] % ref.ROWS, np.arange(n)[None, :] % ref.COLS])


# ------------------------------------------------------------------ the one-hot cases


def _one_nonzero_code_per_row(codes):
    return ((codes != 0).sum(axis=1) == 1).all()


@pytest.mark.parametrize("fmt", [ref.FP8, ref.FP4])
def test_all_codes_case_is_exact_in_fp32(fmt):
    a, bt, sa, sbt, want = ref.all_codes_case(fmt)
    k = a.shape[1] * (2 if fmt == ref.FP4 else 1)
    assert a.shape[0] == bt.shape[0] == 256 and k == (128 if fmt == ref.FP4 else 64)
    assert sa.shape == sbt.shape == (256, k // 32)
    assert min(sa.min(), sbt.min()) >= 119 and max(sa.max(), sbt.max()) <= 135
    assert len(np.unique(sa)) == len(np.unique(sbt)) == 17  # every scale 119 .. 135 occurs
    # one non-zero byte per row of A (row 0 of FP8 and rows 0 mod 16 of FP4 hold code 0: none)
    nz = (a != 0).sum(axis=1)
    zero_rows = np.arange(256) % (16 if fmt == ref.FP4 else 256) == 0
    assert np.array_equal(nz, np.where(zero_rows, 0, 1))
    if fmt == ref.FP8:
        assert np.array_equal(a[np.arange(256), np.arange(256) % 64], np.arange(256))
        assert all((bt[j] == j).all() for j in range(256))
        nan = np.isin(np.arange(256), [0x7F, 0xFF])
    else:
        nib = np.stack([a & 15, a >> 4], axis=-1).reshape(256, 128)
        assert np.array_equal(nib[np.arange(256), np.arange(256) % 128], np.arange(256) % 16)
        assert all((bt[j] == (j % 16) * 0x11).all() for j in range(256))
        nan = np.zeros(256, dtype=bool)
    # NaN exactly in the rows and columns of the two NaN codes; every other value survives fp32
    assert np.array_equal(np.isnan(want), nan[:, None] | nan[None, :])
    fin = want[~np.isnan(want)]
    assert np.array_equal(fin.astype(np.float32).astype(np.float64), fin)
    with np.errstate(invalid="ignore"):
        full = ref.product(fmt, a, bt, sa, sbt)
    assert np.array_equal(np.isnan(full), np.isnan(want)) and np.array_equal(full[~np.isnan(want)], fin)
    # also times 2^±16, the widest scales a pair of blocks could add beyond the seeded ones
    for s in (2.0 ** 16, 2.0 ** -16):
        assert np.array_equal((fin * s).astype(np.float32).astype(np.float64), fin * s)
    if fmt == ref.FP8:  # all 254² finite pairs are there, each a product of the decoded codes
        d = ref.code_values(ref.FP8)
        assert np.isfinite(d).sum() == 254 and fin.size == 254 * 254
        e = np.log2(np.abs(want[0x38, 0x38]))
        assert e == int(e) and -16 <= e <= 16  # 1.0 · 1.0 · the two scales


def test_e8m0_range_case_is_powers_of_two():
    a, bt, sa, sbt, want = ref.e8m0_range_case()
    assert a.shape == bt.shape == (256, ref.E8M0_K) and sa.shape == sbt.shape == (256, ref.E8M0_K // 32)
    assert _one_nonzero_code_per_row(a) and (a[np.arange(256), 32 * np.arange(256)] == 0x38).all()
    assert (bt == 0x38).all()
    hot = sa[np.arange(256), np.arange(256)]
    assert hot.tolist() == [1] + list(range(1, 255)) + [254]  # every byte 1 .. 254 scales an element
    assert min(sa.min(), sbt.min()) >= 1 and max(sa.max(), sbt.max()) <= 254
    # every block's pair of scales stays within 2^±20, whichever row and column meet in it
    pair = sa[0].astype(np.int64)[None, :] + sbt.astype(np.int64) - 254
    assert (sa == sa[0]).all() and pair.min() >= -20 and pair.max() <= 20
    m, e = np.frexp(want)
    assert (m == 0.5).all() and (e - 1).min() >= -20 and (e - 1).max() <= 20  # normal powers of two
    assert len(np.unique(e)) == 41
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert np.array_equal(ref.product(ref.FP8, a, bt, sa, sbt), want)
