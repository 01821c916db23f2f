"""The converter step of the start-up probe, without a GPU.

* the controller: the ``cvt`` token of ``amd.com/gpu-probe`` and ``GPU_PROBE_CVT``, with every value
  accepted before producing the arguments it produced;
* ``odh-gpu-probe --cvt``: its usage errors and the no-GPU verdict;
* the ctypes mirror of the new constants and signatures against ``gpu_probe.h``;
* the family of the fused check: ``odh_cvt_family`` of the built library against the host model
  (``cvt_reference.py``) bit for bit, its expectations against the model's encoder applied independently
  to its inputs, and what it covers;
* the host model of the quantiser: round trip, the scale rule, saturation, the all-zero block.
"""

from __future__ import annotations

import itertools
import json
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


def test_bf16_model_is_torchs():
    rng = np.random.default_rng(16)
    bits = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    bits = bits[((bits >> 23) & 0xFF != 255) & ((bits >> 23) & 0xFF != 0)]
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(cr.encode(cr.BF16, x).astype(np.uint16), want)
    q, s = cr.quantize(cr.BF16, x.reshape(1, -1)[:, :64])
    assert s is None and np.array_equal(q[0], want[:64])
