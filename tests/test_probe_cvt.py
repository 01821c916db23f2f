"""The converter step of the start-up probe, without a GPU.

* the controller: the ``cvt`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_CVT``, with every value
  accepted before producing the arguments it produced;
* ``odh-gpu-probe --cvt``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants and signatures against ``gpu_probe.h``;
* the family of the fused check: ``odh_cvt_family`` of the built library against the host model
  (``cvt_reference.py``) bit for bit, its expectations against the model's encoder applied independently
  to its inputs, and what it covers;
* the host model of the quantiser: round trip, the scale rule, saturation, the all-zero block, and its
  contract for non-finite and subnormal input against a scalar reimplementation, block by block.
"""

from __future__ import annotations

import itertools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cvt_reference as cr
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


def test_cvt_token_adds_the_step_after_the_others():
    assert nbc.GPU_PROBE_CVT_FORMATS == "fp8,bf8,fp4,fp6,bf6,bf16" == ",".join(gpu.CVT_FORMATS) == ",".join(cr.NAMES)
    assert nbc.GPU_PROBE_CVT_TOKENS == ("cvt",)
    assert "cvt" not in nbc.GPU_PROBE_TOKENS + nbc.GPU_PROBE_MORE_TOKENS + nbc.GPU_PROBE_SPARSE_TOKENS
    assert _args("cvt") == BASE + CVT
    assert _args("cvt", gpus=1) == BASE + CVT
    assert _args("true,cvt") == BASE + CVT
    assert _args("rccl,mxall,dtypes,fp,sparse,cvt") == BASE + RCCL + MX_ALL + DTYPES + FP + SPARSE + CVT
    assert _args(" CVT , dtypes,rccl ") == BASE + RCCL + DTYPES + CVT
    others = {"rccl": RCCL, "mx": MX, "mxall": MX_ALL, "dtypes": DTYPES, "fp": FP, "sparse": SPARSE}
    for r in range(len(others) + 1):
        for subset in itertools.combinations(others, r):
            want = list(BASE)
            for token in ("rccl", "mxall" if "mxall" in subset else "mx", "dtypes", "fp", "sparse"):
                if token in subset:
                    want += others[token]
            assert _args(",".join(subset + ("cvt",))) == want + CVT, subset
            assert _args(",".join(("cvt",) + subset)) == want + CVT, subset
            if subset:
                assert _args(",".join(subset)) == want, subset  # and without it, what it was


def test_operator_switch_adds_cvt_to_every_probed_notebook():
    on = {"GPU_PROBE_CVT": "true"}
    assert _args("true", on) == BASE + CVT
    assert _args("rccl", on) == BASE + RCCL + CVT
    assert _args(None, dict(on, GPU_STARTUP_PROBE="true")) == BASE + CVT
    assert _args(None, on) is None  # it does not turn the probe on
    assert _args("false", dict(on, GPU_STARTUP_PROBE="true")) is None  # "false" still wins
    assert _args("mx", dict(on, GPU_PROBE_SPARSE="true", GPU_PROBE_DTYPES="true")) == BASE + MX + DTYPES + SPARSE + CVT
    assert _args("cvt", {"GPU_PROBE_CVT": "false"}) == BASE + CVT


def test_unknown_token_ignores_the_whole_value():
    for value in ("cvt,bogus", "false,cvt", "cvt,", "convert", "cvts"):
        assert _args(value) is None, value
        assert _args(value, {"GPU_STARTUP_PROBE": "true"}) == BASE, value


@pytest.mark.parametrize("cvt_on", [False, True])
def test_values_accepted_before_keep_their_args(cvt_on):
    """Every value the earlier steps' tests list, with the arguments they list for it; under
    ``GPU_PROBE_CVT=true`` each probed one gains ``--cvt`` at the end."""
    on = {"GPU_PROBE_CVT": "true"} if cvt_on else {}

    def check(value, env, want, **kw):
        assert _args(value, dict(env, **on), **kw) == (want + CVT if cvt_on and want is not None else want), \
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
                  "sparse,bogus", "false,sparse", "sparse,", "sparsity", "smfmac"):
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


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_CVT=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_CVT=false\n" in f.read()


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
    ("--cvt", "bogus"), ("--cvt", "fp8,bogus"), ("--cvt", "f32"), ("--cvt", "f16"), ("--cvt", ""), ("--cvt", "fp8,"),
    ("--cvt", "bf16,bf16"), ("--cvt", "fp8,bf8,fp8"), ("--cvt",),
    ("--inject-fault", "cvt"), ("--sparse", "bf16", "--inject-fault", "cvt"), ("--inject-fault", "convert")])
def test_program_cvt_usage_errors(args):
    r = _run(*args)
    assert r.returncode == probe_main.USAGE and r.stdout == "", (args, r.stdout, r.stderr)
    assert "[--cvt fp8,bf8,fp4,fp6,bf6,bf16]" in r.stderr and "[--sparse bf16,f16,i8,fp8,bf8]" in r.stderr
    assert "rccl|mx|dtypes|fp]" in r.stderr and "[--inject-fault sparse]" in r.stderr
    assert "[--inject-fault cvt]" in r.stderr


def test_program_no_gpu_verdict_with_cvt():
    r = _run("--cvt", "fp8,bf8,fp4,fp6,bf6,bf16")
    assert r.returncode == probe_main.NO_GPU
    res = json.loads(r.stdout)
    assert res["ok"] is False and res["error"].startswith("no GPU") and "cvt" not in res
    # accepted next to the other steps, in any order, one format alone, and with its fault hook
    assert _run("--cvt", "bf16,fp4", "--mx", "fp8,fp4", "--sparse", "bf8,i8").returncode == probe_main.NO_GPU
    assert _run("--sparse", "fp8,bf16", "--dtypes", "f16,i8", "--mx", "fp8,fp4,bf8,fp6,bf6", "--fp", "f32,f64",
                "--cvt", "fp6", "--inject-fault", "cvt").returncode == probe_main.NO_GPU
    assert _run("--cvt=bf6", "--inject-fault=cvt").returncode == probe_main.NO_GPU
    # the step uses no operand: it puts no condition on the shape
    assert _run("--cvt", "fp8", "--shape", "256,256,64").returncode == probe_main.NO_GPU


# ------------------------------------------------------------------ ABI mirror


def test_constants_and_signatures_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc", "gpu_probe.h"),
              encoding="utf-8") as f:
        text = f.read()
    header = {k: int(v) for k, v in re.findall(r"^\s*(ODH_CVT_\w+)\s*=\s*(\d+)\s*,", text, re.M)}
    assert header == {"ODH_CVT_FP8": 0, "ODH_CVT_BF8": 1, "ODH_CVT_FP6": 2, "ODH_CVT_BF6": 3, "ODH_CVT_FP4": 4,
                      "ODH_CVT_BF16": 5, "ODH_CVT_BLOCKS": 256, "ODH_CVT_TABLE": 256}
    for name, value in header.items():
        assert getattr(gpu, name) == value, name
    # the scaled formats reuse the hardware's codes, as the MX kernels do
    for name in ("FP8", "BF8", "FP6", "BF6", "FP4"):
        assert getattr(gpu, "ODH_CVT_" + name) == getattr(gpu, "ODH_MX_" + name) == getattr(cr, name) == getattr(mx, name)
    assert gpu.CVT_FORMATS == cr.NAMES and len(set(gpu.CVT_FORMATS.values())) == 6
    params = {"odh_cvt_family_size": 1, "odh_cvt_family": 6, "odh_cvt_fill": 3, "odh_cvt_encode": 7,
              "odh_cvt_quantize": 7, "odh_cvt_probe_verify": 4}
    for name, n in params.items():
        assert len(gpu.SIGNATURES[name][1]) == n, name
        assert re.search(r"\b%s\(" % name, text), name


def test_entry_points_check_their_format_before_anything_else():
    for bad in ("f16", "fp16", "i8", 6, -1):
        for fn in (gpu.cvt_family_size, gpu.cvt_family):
            with pytest.raises(ValueError):
                fn(bad)
    lib = gpu.load_library()
    assert lib.odh_cvt_family_size(6) == 0 and lib.odh_cvt_family_size(-1) == 0
    buf = torch.zeros(8, dtype=torch.int32)
    p = buf.data_ptr()
    size = lib.odh_cvt_family_size(gpu.ODH_CVT_FP4)
    for args in ((6, 0, 1, p, p, p), (gpu.ODH_CVT_FP4, size, 1, p, p, p), (gpu.ODH_CVT_FP4, size - 4, 5, p, p, p),
                 (gpu.ODH_CVT_FP4, 0, 1, None, p, p), (gpu.ODH_CVT_FP4, 0, 1, p, None, p),
                 (gpu.ODH_CVT_FP4, 0, 1, p, p, None)):
        assert lib.odh_cvt_family(*args) == -1, args
    assert not buf.any()
    with pytest.raises(ValueError):
        gpu.cvt_family("fp4", size - 4, 5)
    tail = gpu.cvt_family("fp4", size - 4, 4)
    assert np.array_equal(tail["expect"].numpy(), cr.family(cr.FP4)["expect"][-4:])
    # tensors that are not on a GPU are refused before the library is asked
    x = torch.zeros((2, 32))
    for fn in (lambda: gpu.mx_quantize("fp8", x), lambda: gpu.cvt_encode("fp8", x, torch.zeros((2, 1), dtype=torch.uint8)),
               lambda: gpu.cvt_fill("fp8", torch.zeros(256, dtype=torch.uint8)),
               lambda: gpu.cvt_verify("fp8", torch.zeros(256, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            fn()


# ------------------------------------------------------------------ the family


@pytest.fixture(scope="module", params=list(cr.NAMES))
def fam(request):
    """A format's family from the host model, once."""
    return request.param, cr.NAMES[request.param], cr.family(cr.NAMES[request.param])


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_library_family_is_the_models(fam):
    name, fmt, want = fam
    assert gpu.cvt_family_size(name) == len(want["x"]) == gpu.load_library().odh_cvt_family_size(fmt)
    got = gpu.cvt_family(name)
    assert np.array_equal(_bits(got["x"].numpy()), _bits(want["x"]))  # -0 and +0 differ here
    for key in ("scale", "sel", "expect"):
        assert np.array_equal(got[key].numpy(), want[key]), key
    part = gpu.cvt_family(fmt, 1000, 77)
    assert np.array_equal(_bits(part["x"].numpy()), _bits(want["x"][1000:1077]))


def test_family_expectations_are_the_encoders(fam):
    """By construction on one side, by rounding the exact quotient on the other."""
    _, fmt, f = fam
    assert np.array_equal(cr.encode(fmt, f["x"], f["scale"]), f["expect"])


def test_family_inputs_are_normal_finite_f32(fam):
    _, _, f = fam
    x = f["x"]
    mag = np.abs(x)
    assert np.isfinite(x).all()
    assert ((mag == 0) | (mag >= np.finfo(np.float32).tiny)).all()
    bits = _bits(x)
    assert (((bits >> 23) & 0xFF) != 255).all()
    # zeros are the two exact cases of code 0 and their padding, nothing that underflowed
    assert (f["expect"][mag == 0] & ~(1 << cr.sign_bit(fam[1])) == 0).all()


def test_family_covers_codes_ties_selects_and_scales(fam):
    _, fmt, f = fam
    sign = 1 << cr.sign_bit(fmt)
    want = f["expect"]
    if fmt == cr.BF16:
        finite = np.arange(0x80, 0x7F80)  # every normal bf16 magnitude
        for s in (0, sign):
            assert np.isin(finite | s, want).all()
        assert (0x7F80 in want) and (0xFF80 in want)  # the largest finite bf16 rounds up to infinity
        tie = (_bits(f["x"]) & 0xFFFF) == 0x8000
        c = _bits(f["x"])[tie] >> 16 & 0x7FFF
        assert ((want[tie] & 0x7FFF) == c + (c & 1)).all() and (c & 1).any() and not (c & 1).all()
        assert set(np.unique(_bits(f["x"]) >> 23 & 0xFF).tolist()) == set(range(1, 255))
        return
    cmax, nsel = cr.CMAX[fmt], cr.NSEL[fmt]
    lo, hi = cr.scale_range(fmt)
    assert set(np.unique(f["scale"]).tolist()) == set(range(lo + 127, hi + 128)) and 1 <= lo + 127 and hi + 127 <= 254
    vals, steps, codes = cr.variants(fmt)
    ties = (steps == 0) & ~np.isin(vals, cr.magnitudes(fmt)) & (vals < cr.overflow_midpoint(fmt))
    assert ties.sum() == cmax
    up = codes[ties] == np.arange(cmax) + 1
    assert up.any() and not up.all() and (codes[ties] % 2 == 0).all()  # both directions, always to the even code
    assert np.array_equal(up, np.arange(cmax) % 2 == 1)
    # every select and every scale sees every finite code in both signs, and the overflow class
    shape = (hi - lo + 1, nsel, 2, len(vals))
    e = want.reshape(shape)
    assert (f["sel"].reshape(shape) == np.arange(nsel)[None, :, None, None]).all()
    every = np.concatenate([np.arange(cmax + 1), np.arange(cmax + 1) | sign])
    for si in (0, shape[0] // 2, shape[0] - 1):
        for sel in range(nsel):
            assert np.isin(every, e[si, sel]).all(), (si, sel)
    assert (e == e[0]).all()  # the scale changes no expectation
    tie_code, beyond = cr.OVERFLOW[fmt]
    n = cmax + 1 + 3 * cmax
    assert codes[n:n + 4].tolist() == [cmax, tie_code, beyond, beyond]
    assert (vals[n:n + 3] == cr.overflow_midpoint(fmt)).all() and steps[n:n + 3].tolist() == [-1, 0, 1]
    assert len(vals) % 16 == 0 and 2 * len(vals) % 32 == 0  # 32 consecutive cases share their scale


def test_case_counts_of_the_construction():
    """Codes, and three neighbours of every midpoint: the counts the construction was first checked at."""
    per_scale = {cr.FP8: 505, cr.BF8: 493, cr.FP4: 29, cr.FP6: 125, cr.BF6: 125}
    for fmt, n in per_scale.items():
        assert cr.CMAX[fmt] + 1 + 3 * cr.CMAX[fmt] == n
        assert len(cr.variants(fmt)[0]) == (n + 4 + 15) // 16 * 16
    assert cr.scale_range(cr.FP8) == (-115, 117)
    assert {f: cr.emax(f) for f in cr.SCALED} == {cr.FP8: 8, cr.BF8: 15, cr.FP4: 2, cr.FP6: 2, cr.BF6: 4}
    assert [cr.magnitudes(f)[-1] for f in (cr.FP8, cr.BF8, cr.FP4, cr.FP6, cr.BF6)] == [448, 57344, 6, 7.5, 28]


# ------------------------------------------------------------------ the encoder and the quantiser model


@pytest.mark.parametrize("fmt", cr.SCALED)
def test_encoder_is_nearest_even_against_a_search(fmt):
    """Independent of the encoder's arithmetic: the nearest finite value by exhaustive search over the
    format's values, ties to the even code, for seeded f32 inside the finite range."""
    rng = np.random.default_rng(77 + fmt)
    v = cr.magnitudes(fmt)
    x = (rng.uniform(-1, 1, 4000) * v[-1] * 2.0 ** -rng.integers(0, 12, 4000)).astype(np.float32)
    got = cr.encode(fmt, x)
    d = np.abs(np.abs(x.astype(np.float64))[:, None] - v[None, :])
    best = d.min(axis=1)
    near = d == best[:, None]
    two = near.sum(axis=1) == 2
    lo = near.argmax(axis=1)
    code = np.where(two, lo + (lo & 1), lo)  # of two neighbours c, c + 1 the even one
    assert np.array_equal(got & ~(1 << cr.sign_bit(fmt)), code)
    assert np.array_equal(got >> cr.sign_bit(fmt), np.signbit(x).astype(np.int64))
    # a scale is an exact division
    assert np.array_equal(cr.encode(fmt, np.ldexp(x, 9), 136), got)


@pytest.mark.parametrize("fmt", cr.SCALED)
def test_quantize_round_trips_representable_values(fmt):
    """Blocks of representable values times a power of two, the largest magnitude present: the scale is
    that power of two and the codes are the values'."""
    rng = np.random.default_rng(5 + fmt)
    v = cr.magnitudes(fmt)
    rows, k = 6, 96
    codes = rng.integers(0, len(v), size=(rows, k))
    codes[:, ::32] = cr.CMAX[fmt]  # amax of every block is the largest value
    e = rng.integers(-20, 21, size=(rows, k // 32))
    x = (v[codes] * np.where(rng.random((rows, k)) < 0.5, -1, 1) * 2.0 ** np.repeat(e, 32, axis=1)).astype(np.float32)
    q, s = cr.quantize(fmt, x)
    assert q.shape == (rows, gpu.mx_row_bytes(fmt, k)) and q.dtype == np.uint8 and s.shape == (rows, k // 32)
    assert np.array_equal(s, (e + 127).astype(np.uint8))
    assert np.array_equal(mx.scaled(fmt, q, s), x.astype(np.float64))


@pytest.mark.parametrize("fmt", cr.SCALED)
def test_quantize_scale_rule_saturation_and_zero_blocks(fmt):
    em, top = cr.emax(fmt), cr.magnitudes(fmt)[-1]
    x = np.zeros((5, 32), dtype=np.float32)
    x[0, 3] = 2.0 ** 10  # amax a power of two: floor(log2) is its exponent
    x[1, 3] = np.nextafter(np.float32(2.0 ** 10), np.float32(0))  # just below it: one less
    x[2, 5], x[2, 6] = -1.99 * 2.0 ** em, 1.0  # beyond the overflow midpoint of every format at the block's scale
    x[4, 0] = np.float32(2.0 ** -140)  # a subnormal amax: the smallest scale
    q, s = cr.quantize(fmt, x)
    assert s[:, 0].tolist() == [10 - em + 127, 9 - em + 127, 127, 127, 0]
    val = mx.scaled(fmt, q, s)
    assert val[0, 3] == 2.0 ** 10 and (np.delete(val[0], 3) == 0).all()
    assert val[2, 5] == -top and val[2, 6] == 1.0  # saturated, not NaN or infinity
    assert 1.99 * 2.0 ** em > cr.overflow_midpoint(fmt)
    assert not q[3].any() and s[3, 0] == 127  # an all-zero block: 2^0 and +0
    assert np.isfinite(val).all()
    # what the bare converter makes of the same value is the recorded overflow answer
    raw = cr.encode(fmt, np.float32(1.99 * 2.0 ** em))
    assert int(raw) == cr.OVERFLOW[fmt][1]
    assert cr.mx_scales(fmt, np.full((1, 32), 3e38, dtype=np.float32))[0, 0] == 127 + 127 - em  # no clamp needed above


def _contract_block(fmt, block):
    """One block of 32 by the contract's sentences (``gpu.mx_quantize``), element by element in Python floats:
    ``(byte, codes)``.  Only a finite, already clamped element goes through the model's encoder."""
    em, top, cmax, sign = cr.emax(fmt), float(cr.magnitudes(fmt)[-1]), cr.CMAX[fmt], cr.sign_bit(fmt)
    flt_max = float(np.finfo(np.float32).max)
    block = [float(v) for v in block]
    counted = [min(abs(v), flt_max) for v in block if not math.isnan(v)]  # ±Inf counts as FLT_MAX
    amax = max(counted, default=0.0)
    if amax == 0:  # nothing but NaN, or all zero
        byte = 127
    else:
        byte = min(max(math.frexp(amax)[1] - 1 - em + 127, 0), 254)  # amax = m · 2^e, 0.5 <= m < 1
    lim = top * 2.0 ** (byte - 127)
    codes = []
    for v in block:
        neg = math.copysign(1.0, v) < 0
        if math.isnan(v):
            codes.append(cr.NAN_CODE[fmt] if fmt in cr.NAN_CODE else cmax | neg << sign)
        elif math.isinf(v):
            codes.append(cmax | neg << sign)
        else:
            c = np.float32(min(max(v, -lim), lim))
            assert float(c) == min(max(v, -lim), lim)  # the clamp is exact in f32
            codes.append(int(cr.encode(fmt, c, byte)))
    return byte, codes


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _edge_blocks():
    """Blocks of 32 f32 around every sentence of the contract, and seeded ones with non-finite elements."""
    rng = np.random.default_rng(321)
    inf, nan, flt_max, tiny = np.float32(np.inf), np.float32(np.nan), np.finfo(np.float32).max, np.float32(2.0 ** -149)
    snan, qnan_neg = _f32(0x7F800001), _f32(0xFFC00000)
    base = (rng.standard_normal(32) * 8).astype(np.float32)
    blocks = []

    def put(**at):
        b = base.copy()
        for k, v in at.items():
            b[int(k[1:])] = v
        blocks.append(b)

    blocks.append(np.zeros(32, dtype=np.float32))
    blocks.append(np.full(32, nan))
    blocks.append(np.full(32, -0.0, dtype=np.float32))
    for v in (inf, -inf):
        b = np.zeros(32, dtype=np.float32)
        b[7] = v
        blocks.append(b)
        put(p3=v)
        put(p3=v, p9=flt_max, p10=-flt_max)
    for v in (nan, -nan, snan, -snan, qnan_neg):
        put(p0=v)
        put(p31=v, p4=inf)
        b = np.zeros(32, dtype=np.float32)
        b[11] = v
        blocks.append(b)  # a NaN and zeros: byte 127
    b = np.full(32, nan)
    b[::3] = inf
    b[1::6] = -inf
    blocks.append(b)  # NaN and Inf only
    blocks.append(np.full(32, flt_max))
    blocks.append(np.full(32, tiny))  # the smallest subnormal: byte 0
    for e in (-149, -140, -127, -126, -120, -112, -105, 100, 120, 127):
        b = (base * np.float32(2.0 ** -5)).astype(np.float64) * 2.0 ** e
        with np.errstate(over="ignore", under="ignore"):
            blocks.append(np.clip(b, -flt_max, flt_max).astype(np.float32))
    for _ in range(40):  # seeded bit patterns: every exponent field, 255 included
        b = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
        blocks.append(b)
        b = (b.view(np.uint32) & 0x83FFFFFF | 0x3C000000).view(np.float32).copy()  # a narrow range
        b[rng.integers(0, 32)] = rng.choice([inf, -inf, nan, snan])
        blocks.append(b)
    return np.stack(blocks)


@pytest.mark.parametrize("fmt", cr.SCALED)
def test_quantize_is_the_contract_block_by_block(fmt):
    x = _edge_blocks()
    assert np.isnan(x).any() and np.isinf(x).any() and len(x) > 100
    with np.errstate(invalid="ignore"):
        q, s = cr.quantize(fmt, x)
        codes = mx.unpack(fmt, q)
    assert s.shape == (len(x), 1) and codes.shape == x.shape
    for i, block in enumerate(x):
        byte, want = _contract_block(fmt, block)
        assert int(s[i, 0]) == byte, (i, block)
        assert codes[i].tolist() == want, (i, block)
    # reshaped to three blocks a row the blocks are the same blocks
    n = len(x) // 3 * 3
    with np.errstate(invalid="ignore"):
        q3, s3 = cr.quantize(fmt, x[:n].reshape(-1, 96))
    assert np.array_equal(s3.reshape(-1), s[:n, 0]) and np.array_equal(mx.unpack(fmt, q3).reshape(-1, 32), codes[:n])
    assert s.max() == 254 - cr.emax(fmt) and s.min() == 0 and (s != 255).all()


@pytest.mark.parametrize("fmt", cr.SCALED)
def test_quantize_contract_of_non_finite_elements(fmt):
    """The contract's sentences one by one, as numbers."""
    em, cmax, sign = cr.emax(fmt), cr.CMAX[fmt], 1 << cr.sign_bit(fmt)
    nan_pos, nan_neg = (cr.NAN_CODE[fmt],) * 2 if fmt in cr.NAN_CODE else (cmax, cmax | sign)
    x = np.zeros((6, 32), dtype=np.float32)
    x[0, 4] = np.inf  # alone among zeros
    x[1] = np.linspace(-3, 3, 32)
    x[1, 2], x[1, 20] = -np.inf, np.finfo(np.float32).max  # among finite values, FLT_MAX one of them
    x[2] = x[3] = np.linspace(-3, 3, 32)
    x[2, 6], x[2, 9] = _f32(0x7F800001), _f32(0xFFC00000)  # NaN of both signs among finite values
    x[3, 6], x[3, 9] = 0, 0  # the same block without them
    x[4] = np.nan
    x[5, ::2], x[5, 1::2] = np.nan, -np.inf
    with np.errstate(invalid="ignore"):
        q, s = cr.quantize(fmt, x)
        c = mx.unpack(fmt, q).astype(np.int64)
    assert s[:, 0].tolist() == [254 - em, 254 - em, s[3, 0], s[3, 0], 127, 254 - em] and s[3, 0] == 127 + 1 - em
    assert c[0, 4] == cmax and not np.delete(c[0], 4).any()
    assert c[1, 2] == cmax | sign and c[1, 20] == cmax  # Inf and FLT_MAX saturate alike
    assert set(np.delete(c[1], [2, 20]).tolist()) <= {0, sign}  # 3 / 2^(127 - emax) is far below half a step
    assert c[2, 6] == nan_pos and c[2, 9] == nan_neg
    assert np.array_equal(np.delete(c[2], [6, 9]), np.delete(c[3], [6, 9]))  # the finite neighbours are unchanged
    assert (c[4] == nan_pos).all()
    assert (c[5, ::2] == nan_pos).all() and (c[5, 1::2] == (cmax | sign)).all()
    # what the encoder records beside it
    assert int(cr.encode(fmt, np.float32(np.inf), 127)) == cr.OVERFLOW[fmt][1]  # the bare instruction does not saturate
    every = (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        at255 = cr.encode(fmt, every, 255)
    assert (at255 == cr.SCALE_NAN_CODE[fmt] | (0 if fmt in cr.NAN_CODE else np.signbit(every) * sign)).all()
    assert np.array_equal(at255, cr.encode(fmt, np.where(np.signbit(every), -np.float32(np.nan), np.float32(np.nan))))
    assert cr.SCALE_NAN_CODE[fmt] == (cr.NAN_CODE[fmt] if fmt in cr.NAN_CODE else cmax)


def test_f32_subnormal_inputs_at_the_smallest_scales():
    """An f32 subnormal is not zero to the converter at scale bytes 0 and 1: 2^-127 / 2^-126 is 0.5."""
    x = np.float32(2.0 ** -127)
    assert int(cr.encode(cr.FP8, x, 1)) == 0x30 and int(cr.encode(cr.FP8, -x, 0)) == 0x38 | 0x80
    assert int(cr.encode(cr.FP4, x, 1)) == 1 and int(cr.encode(cr.FP4, x, 0)) == 2
    assert int(cr.encode(cr.FP8, x, 20)) == 0  # and below half the smallest subnormal from there on


def test_bf16_model_keeps_inf_and_quiets_nan():
    x = _f32([0x7F800000, 0xFF800000, 0x7F800001, 0xFF80FFFF, 0x7FC00000, 0xFFFFFFFF, 0x7F7FFFFF, 0x7F7F7FFF,
              0x00000001, 0x00008000, 0x00008001, 0x807FFFFF, 0x00018000])
    want = [0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7FC0, 0xFFFF, 0x7F80, 0x7F7F, 0, 0, 1, 0x8080, 2]
    assert cr.encode(cr.BF16, x).tolist() == want
    got = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    finite = np.isfinite(x)
    assert np.array_equal(got[finite], np.array(want, dtype=np.uint16)[finite])  # torch agrees off the NaNs
    assert np.isnan(x[2:6]).all() and all(w & 0x7FFF > 0x7F80 for w in want[2:6])


def test_bf16_model_is_torchs():
    rng = np.random.default_rng(16)
    bits = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    bits = bits[((bits >> 23) & 0xFF != 255) & ((bits >> 23) & 0xFF != 0)]
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(cr.encode(cr.BF16, x).astype(np.uint16), want)
    q, s = cr.quantize(cr.BF16, x.reshape(1, -1)[:, :64])
    assert s is None and np.array_equal(q[0], want[:64])
