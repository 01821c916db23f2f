"""The 16×16 matrix-core step of the start-up probe, without a GPU.

* the controller: the ``mfma16`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_MFMA16``, with every value
  accepted before producing the arguments it produced;
* ``odh-gpu-probe --mfma16``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants and signatures against ``gpu_probe.h``, and ``m16_shape_ok`` at the stage
  boundaries;
* the host model (``mfma16_reference.py``): each format's lane map tiles the instruction's K exactly once per row,
  the model's instruction equals the plain product, and the scale byte of every (lane, ``opsel``) lands on one block.
"""

from __future__ import annotations

import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mfma16_reference as m16
import mx_reference as mx
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
M16 = ["--mfma16", "bf16,f16,i8,fp8,fp4"]


def test_mfma16_token_adds_the_step_after_the_others():
    assert nbc.GPU_PROBE_MFMA16_FORMATS == "bf16,f16,i8,fp8,fp4" == ",".join(gpu.M16_FORMATS) == ",".join(m16.FORMATS)
    assert nbc.GPU_PROBE_MFMA16_TOKENS == ("mfma16",)
    assert "mfma16" not in (nbc.GPU_PROBE_TOKENS + nbc.GPU_PROBE_MORE_TOKENS + nbc.GPU_PROBE_SPARSE_TOKENS
                            + nbc.GPU_PROBE_CVT_TOKENS + nbc.GPU_PROBE_LDS_TOKENS)
    assert nbc.GPU_PROBE_LDS_TOKENS == ("lds",)
    assert _args("mfma16") == BASE + M16
    assert _args("mfma16", gpus=1) == BASE + M16
    assert _args("true,mfma16") == BASE + M16
    assert _args("rccl,mxall,dtypes,fp,sparse,cvt,lds,mfma16") == \
        BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE + CVT + LDS + M16
    assert _args(" MFMA16 , dtypes,rccl ") == BASE + RCCL + DTYPES + M16
    others = {"rccl": RCCL, "mx": MX, "mxall": MX_ALL, "dtypes": DTYPES, "fp": FP, "sparse": SPARSE, "cvt": CVT,
              "lds": LDS}
    for r in range(len(others) + 1):
        for subset in itertools.combinations(others, r):
            want = list(BASE)
            for token in ("rccl", "mxall" if "mxall" in subset else "mx", "dtypes", "fp", "sparse", "cvt", "lds"):
                if token in subset:
                    want += others[token]
            assert _args(",".join(subset + ("mfma16",))) == want + M16, subset
            assert _args(",".join(("mfma16",) + subset)) == want + M16, subset
            if subset:
                assert _args(",".join(subset)) == want, subset  # and without it, what it was


def test_operator_switch_adds_mfma16_to_every_probed_notebook():
    on = {"GPU_PROBE_MFMA16": "true"}
    assert _args("true", on) == BASE + M16
    assert _args("rccl", on) == BASE + RCCL + M16
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + M16
    assert _args(None, on) is None  # it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("mx", dict(on, GPU_PROBE_LDS="true", GPU_PROBE_DTYPES="true")) == BASE + MX + DTYPES + LDS + M16
    assert _args("mfma16", {"GPU_PROBE_MFMA16": "false"}) == BASE + M16


def test_unknown_token_ignores_the_whole_value():
    for value in ("mfma16,bogus", "false,mfma16", "mfma16,", "mfma16_", "mfma", "mfma32", "16x16"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


@pytest.mark.parametrize("m16_on", [False, True])
def test_values_accepted_before_keep_their_args(m16_on):
    """Every value the earlier steps' tests list, ``lds`` among them, with the arguments they list for it; under
    ``GPU_PROBE_MFMA16=true`` each probed one gains ``--mfma16`` at the end."""
    on = {"GPU_PROBE_MFMA16": "true"} if m16_on else {}

    def check(value, env, want, **kw):
        assert _args(value, dict(env, **on), **kw) == (want + M16 if m16_on and want is not None else want), \
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
                  "convert", "cvts", "lds,bogus", "false,lds", "lds,", "lds_", "ld", "shared"):
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
    check("lds", {}, BASE + LDS)
    check("lds", {}, BASE + LDS, gpus=1)
    check("true,lds", {}, BASE + LDS)
    check("rccl,mxall,dtypes,fp,sparse,cvt,lds", {}, BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE + CVT + LDS)
    check(" LDS , dtypes,rccl ", {}, BASE + RCCL + DTYPES + LDS)
    check("true", {"GPU_PROBE_LDS": "true"}, BASE + LDS)
    check("mx", dict(dt_on, GPU_PROBE_CVT="true", GPU_PROBE_LDS="true"), BASE + MX + DTYPES + CVT + LDS)


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_MFMA16=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_MFMA16=false\n" in f.read()


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
    ("--mfma16", "bogus"), ("--mfma16", "bf16,bogus"), ("--mfma16", "bf8"), ("--mfma16", "f32"), ("--mfma16", ""),
    ("--mfma16", "bf16,"), ("--mfma16", "fp8,fp8"), ("--mfma16", "i8,fp4,i8"), ("--mfma16",),
    ("--inject-fault", "mfma16"), ("--lds", "mem", "--inject-fault", "mfma16"), ("--inject-fault", "mfma"),
    # K = 64 is no instruction of fp8 or fp4; at K = 512 some MX classes expect 0
    ("--mfma16", "fp8", "--shape", "256,256,64"), ("--mfma16", "bf16,fp4", "--shape", "256,256,192"),
    ("--mfma16", "fp4", "--shape", "256,256,512"),
    # and the rules every step shares: K in steps of 64, not a multiple of 35
    ("--mfma16", "bf16", "--shape", "256,256,32"), ("--mfma16", "i8", "--shape", "256,256,2240")])
def test_program_mfma16_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert r.stderr.rstrip().endswith("[--mfma16 bf16,f16,i8,fp8,fp4] [--inject-fault mfma16]")
    assert "[--lds mem,tr16,tr8,tr4,tr6,xlane]" in r.stderr and "[--inject-fault lds]" in r.stderr
    assert "[--cvt fp8,bf8,fp4,fp6,bf6,bf16]" in r.stderr and "[--sparse bf16,f16,i8,fp8,bf8]" in r.stderr
    assert "rccl|mx|dtypes|fp]" in r.stderr and "[--inject-fault sparse]" in r.stderr
    assert "[--inject-fault cvt]" in r.stderr


def test_the_refused_k_has_zero_classes():
    assert mx.zero_classes(512) > 0 and gpu.mx_zero_classes(512) == mx.zero_classes(512) and 512 % 35
    assert mx.zero_classes(1024) == 0 and mx.zero_classes(256) == 0


def test_program_no_gpu_verdict_with_mfma16():
    r = _run("--mfma16", "bf16,f16,i8,fp8,fp4")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "mfma16" not in res
    # accepted next to the other steps, in any order, one format alone, and with its fault hook
    assert _run("--mfma16", "fp4,bf16", "--mx", "fp8,fp4", "--lds", "mem").returncode == probe_main.NO_GPU
    assert _run("--sparse", "fp8,bf16", "--dtypes", "f16,i8", "--mx", "fp8,fp4,bf8,fp6,bf6", "--fp", "f32,f64",
                "--cvt", "fp6", "--lds", "tr6", "--mfma16", "i8", "--inject-fault", "mfma16").returncode == \
        probe_main.NO_GPU
    assert _run("--mfma16=f16", "--inject-fault=mfma16").returncode == probe_main.NO_GPU
    # the dense formats ask no more of K than the bf16 GEMM does
    assert _run("--mfma16", "bf16,f16,i8", "--shape", "256,256,64").returncode == probe_main.NO_GPU
    assert _run("--mfma16", "fp8,fp4", "--shape", "256,256,256").returncode == probe_main.NO_GPU
    assert _run("--mfma16", "bf16,i8", "--shape", "256,256,512").returncode == probe_main.NO_GPU  # no MX table asked


# ------------------------------------------------------------------ ABI mirror


def test_constants_and_signatures_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        text = f.read()
    header = {k: int(v) for k, v in re.findall(r"^\s*(ODH_M16_\w+)\s*=\s*(\d+)\s*,", text, re.M)}
    assert header == {"ODH_M16_BF16": 0, "ODH_M16_F16": 1, "ODH_M16_I8": 2, "ODH_M16_FP8": 3, "ODH_M16_FP4": 4}
    for name, value in header.items():
        assert getattr(gpu, name) == value, name
    assert gpu.M16_FORMATS == m16.CODES
    params = {"odh_m16_gemm": 10, "odh_m16_probe_gemm_verify": 12, "odh_m16_one": 9}
    for name, n in params.items():
        assert len(gpu.SIGNATURES[name][1]) == n, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and decl.group(1).count(",") + 1 == n, name


@pytest.mark.parametrize("fmt", m16.FORMATS)
def test_shape_ok_at_the_stage_boundaries(fmt):
    s = m16.STAGE[fmt]
    assert gpu.m16_stage(fmt) == s and gpu.m16_scaled(fmt) == (fmt in m16.SCALED)
    for k, ok in ((s, True), (2 * s, True), (7 * s, True), (s // 2, False), (s + s // 2, False), (s - 1, False),
                  (s + 1, False), (0, False), (-s, False)):
        assert gpu.m16_shape_ok(fmt, 256, 256, k) is ok, k
        assert gpu.m16_shape_ok(gpu.M16_FORMATS[fmt], 512, 768, k) is ok, k
    for m, n in ((128, 256), (256, 128), (0, 256), (256, 384), (255, 256), (-256, 256)):
        assert gpu.m16_shape_ok(fmt, m, n, s) is False, (m, n)
    for bad in ("bf8", "fp6", "f32", "mfma16", 5, -1):
        with pytest.raises(ValueError):
            gpu.m16_shape_ok(bad, 256, 256, 128)


def test_entry_points_check_their_arguments_before_anything_else():
    lib = gpu.load_library()
    invalid = 1  # hipErrorInvalidValue
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    p = buf.data_ptr()
    assert p % 16 == 0
    for fmt, m, n, k in ((5, 256, 256, 128), (-1, 256, 256, 128), (0, 128, 256, 32), (1, 256, 256, 16), (2, 256, 256, 32),
                         (3, 256, 256, 64), (4, 256, 384, 128), (0, 256, 256, 0)):
        sp = p if fmt in (3, 4) else None
        assert lib.odh_m16_gemm(fmt, p, p, sp, sp, p, m, n, k, None) == invalid, (fmt, m, n, k)
        assert lib.odh_m16_probe_gemm_verify(fmt, p, p, sp, sp, sp, m, n, k, None, p, None) == invalid, (fmt, m, n, k)
    # scales or a table with a dense format, none with a scaled one, null or misaligned pointers
    for args in ((0, p, p, p, None), (1, p, p, None, p), (2, p, p, p, p), (3, p, p, None, p), (4, p, p, p, None),
                 (0, None, p, None, None), (0, p, None, None, None), (0, p + 8, p, None, None), (3, p, p + 4, p, p),
                 (3, p, p, p + 2, p), (4, p, p, p, p + 1)):
        fmt, xa, xb, xs, xt = args
        assert lib.odh_m16_gemm(fmt, xa, xb, xs, xt, p, 256, 256, 128, None) == invalid, args
        tab = p if fmt in (3, 4) else None
        assert lib.odh_m16_probe_gemm_verify(fmt, xa, xb, xs, xt, tab, 256, 256, 128, None, p, None) == invalid, args
        assert lib.odh_m16_one(fmt, xa, xb, xs, xt, 0, 0, p, None) == invalid, args
    assert lib.odh_m16_gemm(0, p, p, None, None, None, 256, 256, 128, None) == invalid
    assert lib.odh_m16_probe_gemm_verify(0, p, p, None, None, p, 256, 256, 128, None, p, None) == invalid  # a table
    assert lib.odh_m16_probe_gemm_verify(3, p, p, p, p, None, 256, 256, 128, None, p, None) == invalid  # no table
    assert lib.odh_m16_probe_gemm_verify(0, p, p, None, None, None, 256, 256, 128, None, None, None) == invalid
    for oa, ob in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        assert lib.odh_m16_one(3, p, p, p, p, oa, ob, p, None) == invalid
        assert lib.odh_m16_one(0, p, p, None, None, oa, ob, p, None) == invalid
    assert lib.odh_m16_one(5, p, p, p, p, 0, 0, p, None) == invalid and lib.odh_m16_one(4, p, p, p, p, 0, 0, None, None) == invalid
    assert not buf.any()
    # tensors that are not on a GPU are refused before the library is asked
    a = torch.zeros((256, 128), dtype=torch.bfloat16)
    r = torch.zeros((64, 8), dtype=torch.int32)
    for fn in (lambda: gpu.m16_gemm("bf16", a, a), lambda: gpu.m16_verify("bf16", a, a),
               lambda: gpu.m16_one("bf16", r, r), lambda: gpu.m16_gemm("bf8", a, a)):
        with pytest.raises(ValueError):
            fn()


# ------------------------------------------------------------------ the model


@pytest.mark.parametrize("fmt", m16.FORMATS)
def test_lane_map_tiles_k_exactly_once_per_row(fmt):
    seen = np.zeros((16, m16.STAGE[fmt]), dtype=np.int64)
    for lane in range(64):
        for e in range(m16.ELEMS[fmt]):
            assert 0 <= m16.lane_row(lane) < 16 and 0 <= m16.lane_k(fmt, lane, e) < m16.STAGE[fmt]
            seen[m16.lane_row(lane), m16.lane_k(fmt, lane, e)] += 1
    assert (seen == 1).all()
    assert m16.ELEMS[fmt] * m16.BITS[fmt] == 32 * m16.REGS[fmt] and 4 * m16.ELEMS[fmt] == m16.STAGE[fmt]
    cd = {m16.cd_position(lane, r) for lane in range(64) for r in range(4)}
    assert cd == {(i, j) for i in range(16) for j in range(16)}


@pytest.mark.parametrize("fmt", m16.FORMATS)
def test_model_instruction_is_the_plain_product(fmt):
    rng = np.random.default_rng(5)
    k = m16.STAGE[fmt]
    va, vb = rng.integers(-3, 4, size=(16, k)), rng.integers(-3, 4, size=(16, k))
    a, b = m16.from_matrix(fmt, m16.encode(fmt, va)), m16.from_matrix(fmt, m16.encode(fmt, vb))
    want = (va @ vb.T).astype(np.float64)
    sa = sb = None
    if fmt in m16.SCALED:
        # scale bytes by the public layout [row][block]: lane (r, g) carries block g of row r in byte opsel
        ea, eb = rng.integers(-3, 4, size=(16, 4)), rng.integers(-3, 4, size=(16, 4))
        junk = rng.integers(1, 255, size=(64, 4))
        sa, sb = junk.copy(), junk[::-1].copy()
        for lane in range(64):
            sa[lane, 2], sb[lane, 1] = 127 + ea[lane & 15, lane >> 4], 127 + eb[lane & 15, lane >> 4]
        sa, sb = (x.astype(np.uint8).view(np.int32).reshape(64) for x in (sa, sb))
        want = ((va * np.repeat(2.0 ** ea, 32, axis=1)) @ (vb * np.repeat(2.0 ** eb, 32, axis=1)).T)
    d, mag = m16.one(fmt, a, b, sa, sb, 2, 1)
    for lane in range(64):
        for r in range(4):
            assert d[lane, r] == want[4 * (lane >> 4) + r, lane & 15]
    assert (mag >= np.abs(d)).all()
    # registers ↔ elements round trip, and the unused upper registers stay zero
    assert np.array_equal(m16.registers(fmt, m16.elements(fmt, a)), a)
    assert not a[:, m16.REGS[fmt]:].any()


@pytest.mark.parametrize("fmt", m16.SCALED)
def test_scale_byte_of_every_lane_and_opsel_lands_on_one_block(fmt):
    for opsel in range(4):
        users = {}
        for lane in range(64):
            for e in range(m16.ELEMS[fmt]):
                src = m16.scale_source(fmt, lane, e, opsel)
                assert src[1] == opsel and 0 <= src[0] < 64
                users.setdefault(src, set()).add((m16.lane_row(lane), m16.lane_k(fmt, lane, e) // 32))
        assert len(users) == 64  # every lane's byte is used
        for (lane, _), blocks in users.items():
            assert blocks == {(lane & 15, lane >> 4)}, (lane, blocks)  # by exactly one block: its row's block g
    # fp4: a lane's own elements; fp8: each lane's two register halves take two other lanes' scales
    own = all(m16.scale_source(fmt, lane, e, 0)[0] == lane for lane in range(64) for e in range(m16.ELEMS[fmt]))
    assert own == (fmt == "fp4")
    if fmt == "fp8":
        for lane in range(64):
            g, r = lane >> 4, lane & 15
            assert {m16.scale_source(fmt, lane, e, 0)[0] for e in range(16)} == {r + 16 * (g >> 1)}
            assert {m16.scale_source(fmt, lane, e, 0)[0] for e in range(16, 32)} == {r + 16 * (2 + (g >> 1))}


def test_scale_family_bytes_tell_every_place_apart_over_two_passes():
    places = [(lane, byte) for lane in range(64) for byte in range(4)]
    both = {tuple(m16.scale_byte(lane, byte, w) for w in m16.SCALE_WRAPS) for lane, byte in places}
    assert len(both) == 256
    assert all(1 <= m16.scale_byte(lane, byte, w) <= 254 for lane, byte in places for w in m16.SCALE_WRAPS)
