"""The ``dcvt`` step off the GPU: the controller's token and switch, the generated ``params.env`` files, the host
arithmetic of the family and fault counts that ``tests/test_gpu_dcvt.py`` relies on, and the program's refusals."""

import os
import subprocess

import pytest

from odh_kubeflow_amd.controllers import notebook as nbc
from odh_kubeflow_amd.controllers.notebook import GPU_PROBE_ANNOTATION, generate_statefulset
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.ops import gpu, probe_main

torch = pytest.importorskip("torch")

BASE = ["--json", "/dev/termination-log", "--timeout-ms", "30000"]
VMEM = ["--vmem", "cache,sub,buf,dma"]
DCVT = ["--dcvt", "fp8,bf8,fp4,fp6,bf6"]


def _args(value=None, env=None):
    nb = notebook("nb", "ns", gpus=2, annotations={GPU_PROBE_ANNOTATION: value} if value is not None else None)
    inits = generate_statefulset(nb, False, env or {})["spec"]["template"]["spec"].get("initContainers") or []
    return inits[0]["args"] if inits else None


@pytest.mark.parametrize("value, env, want", [
    ("dcvt", {}, BASE + DCVT),
    ("dcvt,vmem", {}, BASE + VMEM + DCVT),
    (" DCVT , cvt,rccl", {}, BASE + ["--rccl-mib", "64", "--cvt", "fp8,bf8,fp4,fp6,bf6,bf16"] + DCVT),
    ("vmem", {"GPU_PROBE_DCVT": "true"}, BASE + VMEM + DCVT),
    (None, {"GPU_PROBE_DCVT": "true", "GPU_STARTUP_PROBE": "true"}, BASE + DCVT),
    (None, {"GPU_PROBE_DCVT": "true"}, None),  # the switch does not turn the probe on
    ("false", {"GPU_PROBE_DCVT": "true", "GPU_STARTUP_PROBE": "true"}, None),
    # without the token or the variable the arguments are what they were
    ("true", {}, BASE), ("vmem", {"GPU_PROBE_DCVT": "false"}, BASE + VMEM), ("dcvt,bogus", {}, None), ("dcvts", {}, None),
])
def test_dcvt_token_and_switch_add_the_step_after_vmem(value, env, want):
    assert nbc.GPU_PROBE_DCVT_FORMATS == "fp8,bf8,fp4,fp6,bf6" == ",".join(gpu.DCVT_FORMATS)
    assert nbc.GPU_PROBE_DCVT_TOKENS == ("dcvt",) and nbc.GPU_PROBE_VMEM_TOKENS == ("vmem",)
    assert _args(value, env) == want


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_VMEM=false\nGPU_PROBE_DCVT=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_DCVT=false\n" in f.read()


# per format: scale bytes of the float32 (and bfloat16) window, of the float16 one, and per scale the items, the
# values an item compares (float32 of fp8 / bf8: the one-value form too) and of the items those a wrong scale changes:
# all but the zeros and, in fp8 and bf8, the 2 or 8 NaN and infinity codes
FAMILY = {"fp8": (237, 13, 256, (8, 4), 252), "bf8": (223, 0, 256, (8, 4), 246), "fp4": (251, 27, 256, (8, 8), 224),
          "fp6": (249, 25, 64, (32, 32), 62), "bf6": (246, 22, 64, (32, 32), 62)}


@pytest.mark.parametrize("fmt", list(gpu.DCVT_FORMATS))
def test_family_and_fault_counts_of_the_bytes_the_gpu_test_changes(fmt):
    n32, n16, items, (v32, v16), nonzero_items = FAMILY[fmt]
    assert gpu.dcvt_family_size(fmt) == items * ((n32 * v32) + (n16 + n32) * v16)
    waves = gpu.ODH_CVT_BLOCKS * 4
    for byte in (3, 9, 120):
        in16 = 112 <= byte < 112 + n16  # float16's window starts 112 bytes above float32's: emin -14 against -126
        assert gpu.dcvt_fault_count(fmt, byte) == nonzero_items * (v32 + v16 + (v16 if in16 else 0)) * waves, byte
    assert gpu.dcvt_fault_count(fmt, n32 - 1) > 0 == gpu.dcvt_fault_count(fmt, n32) == gpu.dcvt_fault_count(fmt, -1)
    assert gpu.dcvt_fault_count("bf16", 3) == 0 and gpu.dcvt_fault_count(7, 3) == 0
    assert gpu.load_library().odh_dcvt_family_size(gpu.ODH_CVT_BF16) == 0


@pytest.mark.parametrize("formats", ["bogus", "fp8,fp8", "fp8,bf16", ""])
def test_program_refuses_unknown_and_repeated_formats(formats):
    exe = probe_main.executable()
    if not os.path.exists(exe):
        pytest.fail("odh-gpu-probe not built: python -m odh_kubeflow_amd.ops.build")
    r = subprocess.run([exe, "--json", "-", "--dcvt", formats], capture_output=True, text=True, timeout=60)
    assert r.returncode == probe_main.USAGE and r.stdout == "" and "--dcvt fp8,bf8,fp4,fp6,bf6" in r.stderr
    r = subprocess.run([exe, "--json", "-", "--inject-fault", "dcvt"], capture_output=True, text=True, timeout=60)
    assert r.returncode == probe_main.USAGE  # the step's fault needs the step
