"""The BF8 / FP6 / BF6 formats of the start-up probe's block-scaled step, without a GPU.

* the controller: the ``mxall`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_MX_ALL``, with every
  value accepted before producing the arguments it produced;
* ``odh-gpu-probe --mx`` with the new names: its usage errors and the no-GPU verdict;
* the host model (``mx_reference.py``): the decoder on known codes of the three formats, the 6-bit packing,
  and the probe's 15 × 21 table against the full product of the operands as each format
  encodes them;
* the ctypes mirror of the new constants.
"""

from __future__ import annotations

import json
import os
import re
import subprocess

import numpy as np
import pytest

import mx_reference as ref
from odh_kubeflow_amd.controllers import notebook as nbc
from odh_kubeflow_amd.controllers.notebook import (GPU_PROBE_ANNOTATION, GPU_PROBE_CONTAINER, generate_statefulset)
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.ops import gpu, probe_main

FORMATS = ["bf8", "fp6", "bf6"]

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


def test_mxall_token_checks_every_format():
    assert nbc.GPU_PROBE_MX_ALL_FORMATS == "fp8,fp4,bf8,fp6,bf6" and "mxall" in nbc.GPU_PROBE_TOKENS
    assert nbc.GPU_PROBE_MX_FORMATS == "fp8,fp4"
    assert _args("mxall") == BASE + MX_ALL
    assert _args("mx,mxall") == BASE + MX_ALL  # one --mx argument
    assert _args("rccl,mxall,dtypes") == BASE + RCCL + MX_ALL + DTYPES  # where --mx is, before --dtypes
    assert _args(" MXALL , rccl ") == BASE + RCCL + MX_ALL
    assert _args("true,mxall") == BASE + MX_ALL
    assert _args("mxall", gpus=1) == BASE + MX_ALL


def test_operator_switch_checks_every_format_on_every_probed_notebook():
    on = {"GPU_PROBE_MX_ALL": "true"}
    assert _args("true", on) == BASE + MX_ALL
    assert _args("mx", on) == BASE + MX_ALL
    assert _args("rccl,dtypes", on) == BASE + RCCL + MX_ALL + DTYPES
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + MX_ALL
    assert _args(None, on) is None  # like GPU_PROBE_MX, it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("true", dict(on, GPU_PROBE_MX="true")) == BASE + MX_ALL


def test_unknown_token_ignores_the_whole_value():
    assert _args("mxall") == BASE + MX_ALL  # the token itself is known: what follows is about its neighbours
    for value in ("mxall,bogus", "mxall,", "false,mxall", "mx_all", "mx-all"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


def test_values_accepted_before_keep_their_args():
    """Every value ``test_probe_mx.py`` and ``test_probe_dtypes.py`` list, with their arguments, now
    that ``mxall`` and ``GPU_PROBE_MX_ALL`` exist (and with the switch spelled out as off)."""
    assert set(nbc.GPU_PROBE_TOKENS) == {"true", "rccl", "mx", "mxall", "dtypes", "false"}
    off = {"GPU_PROBE_MX_ALL": "false"}
    assert _args("mx", off) == BASE + MX and _args("rccl,mx,dtypes", off) == BASE + RCCL + MX + DTYPES
    assert _args("true") == BASE
    assert _args("rccl") == BASE + RCCL
    assert _args("false", {"GPU_STARTUP_PROBE": "true"}) is None
    assert _args(None) is None and _args(None, {"GPU_STARTUP_PROBE": "true"}) == BASE
    assert _args("mx") == BASE + MX
    assert _args("rccl,mx") == BASE + RCCL + MX
    assert _args(" MX , rccl ") == BASE + RCCL + MX
    assert _args("true,mx") == BASE + MX
    assert _args("mx", gpus=1) == BASE + MX
    assert _args("dtypes") == BASE + DTYPES
    assert _args("rccl,mx,dtypes") == BASE + RCCL + MX + DTYPES
    assert _args("mx,dtypes") == BASE + MX + DTYPES
    mx_on = {"GPU_PROBE_MX": "true"}
    assert _args("true", mx_on) == BASE + MX
    assert _args("rccl", mx_on) == BASE + RCCL + MX
    assert _args(None, dict(mx_on, GPU_STARTUP_PROBE="true")) == BASE + MX
    assert _args(None, mx_on) is None
    assert _args("dtypes", dict(mx_on, GPU_PROBE_DTYPES="true")) == BASE + MX + DTYPES
    for value in ("mx,bogus", "yes", "mx,", "false,mx", "dtypes,bogus"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_MX_ALL=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_MX_ALL=false\n" in f.read()


# ------------------------------------------------------------------ the program


def _exe():
    path = probe_main.executable()
    if not os.path.exists(path):
        pytest.fail("odh-gpu-probe not built: python -m odh_kubeflow_amd.ops.build")
    return path


def _run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # a pod without GPUs (also on a GPU machine)
    return subprocess.run([_exe(), "--json", "-", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args", [("--mx", "fp6,fp6"), ("--mx", "fp8,fp4,bf8,fp6,bf6,bf8"), ("--mx", "fp5"),
                                  ("--mx", "bf6", "--shape", "256,256,192"),   # K is no multiple of 128
                                  ("--mx", "bf8", "--shape", "256,256,512")])  # two classes expect 0 at K = 512
def test_program_new_formats_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert "bf8,fp6,bf6" in r.stderr


@pytest.mark.parametrize("args", [("--mx", "fp8,fp4,bf8,fp6,bf6"), ("--mx", "fp6", "--shape", "256,256,384"),
                                  ("--mx", "bf6,bf8,fp6", "--inject-fault", "mx")])
def test_program_no_gpu_verdict_with_new_formats(args):
    r = _run(*args)
    assert r.returncode == probe_main.NO_GPU, (args, r.stdout, r.stderr)
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "mx" not in res


# ------------------------------------------------------------------ ABI mirror


def test_constants_mirror_the_header_and_the_model():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        header = {k: int(v) for k, v in re.findall(r"\b(ODH_MX_\w+)\s*=\s*(\d+)\s*,", f.read())}
    assert header == {"ODH_MX_FP8": 0, "ODH_MX_BF8": 1, "ODH_MX_FP6": 2, "ODH_MX_BF6": 3, "ODH_MX_FP4": 4,
                      "ODH_MX_CLASSES": 315}
    for name, value in header.items():
        assert getattr(gpu, name) == value, name
    assert gpu.MX_EXTRA_FORMATS == {name: ref.NAMES[name] for name in FORMATS} == {"bf8": 1, "fp6": 2, "bf6": 3}
    assert gpu.MX_FORMATS == {name: ref.NAMES[name] for name in ("fp8", "fp4")} == {"fp8": 0, "fp4": 4}
    assert gpu.MX_ALL_FORMATS == ref.NAMES
    assert (ref.BF8, ref.FP6, ref.BF6) == (gpu.ODH_MX_BF8, gpu.ODH_MX_FP6, gpu.ODH_MX_BF6)
    # shapes: K in stages of 64 (BF8) or 128 (FP6, BF6) elements; rows of 3K/4 bytes when packed
    assert gpu.mx_shape_ok("bf8", 256, 512, 64) and not gpu.mx_shape_ok("bf8", 256, 512, 32)
    for fmt in ("fp6", "bf6"):
        assert gpu.mx_shape_ok(fmt, 256, 512, 128) and not gpu.mx_shape_ok(fmt, 256, 512, 64)
        assert not gpu.mx_shape_ok(fmt, 128, 512, 128)
        assert gpu.mx_row_bytes(fmt, 128) == 96 and gpu.mx_row_bytes(fmt, 1024) == 768
    assert gpu.mx_row_bytes("bf8", 64) == 64 and gpu.mx_row_bytes("fp8", 64) == 64 and gpu.mx_row_bytes("fp4", 128) == 64
    with pytest.raises(ValueError):
        gpu.mx_shape_ok("fp5", 256, 256, 128)


# ------------------------------------------------------------------ the model


def _codes():
    """The format codes the library takes, which are the model's."""
    assert gpu.MX_EXTRA_FORMATS == {name: ref.NAMES[name] for name in FORMATS}
    return gpu.ODH_MX_BF8, gpu.ODH_MX_FP6, gpu.ODH_MX_BF6


def test_decoders_on_known_codes():
    assert _codes() == (ref.BF8, ref.FP6, ref.BF6)
    # the probe's codes of 1, 2, 3 and the sign bit, as the fill encodes them
    assert ref.decode_codes(ref.BF8, [0x00, 0x3C, 0x40, 0x42, 0xC2, 0x80]).tolist() == [0.0, 1.0, 2.0, 3.0, -3.0, -0.0]
    assert ref.decode_codes(ref.FP6, [0x00, 0x08, 0x10, 0x14, 0x34, 0x20]).tolist() == [0.0, 1.0, 2.0, 3.0, -3.0, -0.0]
    assert ref.decode_codes(ref.BF6, [0x00, 0x0C, 0x10, 0x12, 0x32, 0x20]).tolist() == [0.0, 1.0, 2.0, 3.0, -3.0, -0.0]
    # the maxima, the smallest subnormals, and e5m2's infinities and NaNs
    assert ref.decode_codes(ref.BF8, [0x7B, 0xFB, 0x01, 0x04]).tolist() == [57344.0, -57344.0, 2.0 ** -16, 2.0 ** -14]
    assert ref.decode_codes(ref.BF8, [0x7C, 0xFC]).tolist() == [np.inf, -np.inf]
    assert np.isnan(ref.decode_codes(ref.BF8, [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF])).all()
    assert np.isfinite(ref.decode_codes(ref.BF8, np.arange(0x7C))).all()
    assert ref.decode_codes(ref.FP6, [0x1F, 0x3F, 0x01, 0x07, 0x09]).tolist() == [7.5, -7.5, 0.125, 0.875, 1.125]
    assert ref.decode_codes(ref.BF6, [0x1F, 0x3F, 0x01, 0x03, 0x04, 0x0D]).tolist() == [28.0, -28.0, 2.0 ** -4, 0.1875, 0.25, 1.25]
    for fmt, top in ((ref.FP6, 7.5), (ref.BF6, 28.0)):
        v = ref.code_values(fmt)
        assert np.isfinite(v).all() and v.max() == top and v.min() == -top
        assert np.array_equal(v[32:], -v[:32]) and (np.diff(v[:32]) > 0).all()  # sign-magnitude, monotonic
        assert len(set(v[:32].tolist())) == 32
    # the 31 multiples of 1/2 up to 7.5 (FP6) and the multiples of 1/2 up to 8 that e3m2 holds (BF6)
    half6 = sorted(x for x in set(ref.code_values(ref.FP6).tolist()) if x * 2 == int(x * 2))
    assert half6 == [x / 2 for x in range(-15, 16)]
    halfb = sorted(x for x in set(ref.code_values(ref.BF6).tolist()) if x * 2 == int(x * 2) and abs(x) <= 8)
    assert [x for x in halfb if x > 0] == [0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 5, 6, 7, 8]


def test_packing_round_trips_every_code_at_every_offset():
    assert gpu.mx_row_bytes(_codes()[1], 8) == 6  # the library's row of 8 elements, as packed below
    for off in range(4):  # k mod 4: the four bit offsets 0, 6, 4 and 2 of an element in its byte
        for code in range(64):
            x = np.zeros((1, 8), dtype=np.uint8)
            x[0, off] = code
            x[0, 4 + off] = 63 - code
            p = ref.pack6(x)
            assert p.shape == (1, 6) and np.array_equal(ref.unpack6(p), x), (off, code)
    rng = np.random.default_rng(6)
    x = rng.integers(0, 64, size=(5, 128), dtype=np.uint8)
    p = ref.pack6(x)
    assert p.shape == (5, 96) and p.dtype == np.uint8 and np.array_equal(ref.unpack6(p), x)
    # the layout's definition, bit by bit: element k is bits [6k, 6k + 6) of the row, little endian
    row = int.from_bytes(p[3].tobytes(), "little")
    assert [(row >> (6 * k)) & 63 for k in range(128)] == x[3].tolist()
    # an all-ones element sets only its own six bits
    one = np.zeros((1, 4), dtype=np.uint8)
    one[0, 1] = 63
    assert ref.pack6(one).tolist() == [[0xC0, 0x0F, 0x00]]


def test_set_code_changes_one_element():
    assert gpu.mx_row_bytes(_codes()[2], 128) == 96
    rng = np.random.default_rng(7)
    x = rng.integers(0, 64, size=(3, 128), dtype=np.uint8)
    p = ref.pack6(x)
    for k in (0, 1, 2, 3, 64, 97, 126, 127):
        for code in (0, 63, 0x14, 0x2A):
            q = p.copy()
            ref.set_code(q, 1, k, code)
            y = x.copy()
            y[1, k] = code
            assert np.array_equal(ref.unpack6(q), y), (k, code)


@pytest.mark.parametrize("k", [128, 384, 1024])
@pytest.mark.parametrize("fmt", FORMATS)
def test_table_is_the_product_of_the_encoded_operands(fmt, k):
    code = ref.NAMES[fmt]
    m, n = 30, 42  # two periods of the classes each way
    va, vb = ref.probe_values(m, n, k)
    a, bt = ref.encode(code, va), ref.encode(code, vb)
    assert a.shape == (m, gpu.mx_row_bytes(fmt, k)) and a.dtype == np.uint8
    assert np.array_equal(ref.decode(code, a), va) and np.array_equal(ref.decode(code, bt), vb)
    # the codes the fill writes for 1, 2, 3 and the sign
    codes = ref.unpack6(a) if code in ref.PACKED else a
    one, two, three, sign = {ref.BF8: (0x3C, 0x40, 0x42, 0x80), ref.FP6: (0x08, 0x10, 0x14, 0x20),
                             ref.BF6: (0x0C, 0x10, 0x12, 0x20)}[code]
    assert set(np.unique(codes).tolist()) == {0, one, two, one | sign, two | sign}  # A is -2 .. 2
    assert three in (ref.unpack6(bt) if code in ref.PACKED else bt)
    sa, sbt = ref.probe_scales(m, k), ref.probe_scales(n, k)
    t = ref.probe_table(k)
    want = ref.product(code, a, bt, sa, sbt)
    assert np.array_equal(want, t[np.arange(m)[:, None] % ref.ROWS, np.arange(n)[None, :] % ref.COLS])
    assert (ref.zero_classes(k) == 0) == bool((t != 0).all())


def test_one_hot_cases_are_single_products():
    for fmt in _codes():
        a, bt, sa, sbt, want = ref.all_codes_case(fmt)
        assert want.shape == (256, 256)
        got = ref.product(fmt, a, bt, sa, sbt)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
        fin = want[np.isfinite(want)]
        assert np.array_equal(fin.astype(np.float32).astype(np.float64), fin)  # exact in fp32
        if fmt == ref.BF8:
            assert nan[:, 0x7C].all() and nan[:, 0xFF].all() and nan[0x7D].all()  # 0 · inf over the other 63 k
            assert want[0x7C, 0x3C] == np.inf and want[0x7C, 0xBC] == -np.inf and want[0xFC, 0x3C] == -np.inf
            assert np.isnan(want[0x7C, 0x00]) and np.isnan(want[0x7C, 0x80])
        else:
            codes = ref.unpack6(a)
            hot = np.arange(256) % 128
            assert np.array_equal(codes[np.arange(256), hot], (np.arange(256) + 21 * (np.arange(256) >> 7)) % 64)
            assert (codes != 0).sum(axis=1).max() == 1 and not nan.any()
            assert set(codes[np.arange(256), hot].tolist()) == set(range(64))
    a, bt, sa, sbt, want = ref.e8m0_range_case(ref.FP6)
    assert a.shape == (256, 6144) and set(sa[0].tolist()) == set(range(1, 255))
    assert np.array_equal(ref.unpack6(a)[np.arange(256), 32 * np.arange(256)], np.full(256, 0x08))
    assert np.array_equal(np.log2(want), np.round(np.log2(want))) and want.min() >= 2.0 ** -20
