"""The ``vmem`` step off the GPU: the controller's token and switch, the generated ``params.env`` files, and the
host arithmetic of the fault counts that ``tests/test_gpu_vmem.py`` relies on."""

import os

import pytest

from odh_kubeflow_amd.controllers import notebook as nbc
from odh_kubeflow_amd.controllers.notebook import GPU_PROBE_ANNOTATION, generate_statefulset
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.ops import gpu

torch = pytest.importorskip("torch")

BASE = ["--json", "/dev/termination-log", "--timeout-ms", "30000"]
M16 = ["--mfma16", "bf16,f16,i8,fp8,fp4"]
VMEM = ["--vmem", "cache,sub,buf,dma"]


def _args(value=None, env=None):
    nb = notebook("nb", "ns", gpus=2, annotations={GPU_PROBE_ANNOTATION: value} if value is not None else None)
    inits = generate_statefulset(nb, False, env or {})["spec"]["template"]["spec"].get("initContainers") or []
    return inits[0]["args"] if inits else None


@pytest.mark.parametrize("value, env, want", [
    ("vmem", {}, BASE + VMEM),
    ("vmem,mfma16", {}, BASE + M16 + VMEM),
    (" VMEM , lds,rccl", {}, BASE + ["--rccl-mib", "64", "--lds", "mem,tr16,tr8,tr4,tr6,xlane"] + VMEM),
    ("mfma16", {"GPU_PROBE_VMEM": "true"}, BASE + M16 + VMEM),
    (None, {"GPU_PROBE_VMEM": "true", "GPU_STARTUP_PROBE": "true"}, BASE + VMEM),
    (None, {"GPU_PROBE_VMEM": "true"}, None),  # the switch does not turn the probe on
    ("false", {"GPU_PROBE_VMEM": "true", "GPU_STARTUP_PROBE": "true"}, None),
    # without the token or the variable the arguments are what they were
    ("true", {}, BASE), ("mfma16", {"GPU_PROBE_VMEM": "false"}, BASE + M16), ("vmem,bogus", {}, None), ("vmems", {}, None),
])
def test_vmem_token_and_switch_add_the_step_after_mfma16(value, env, want):
    assert nbc.GPU_PROBE_VMEM_FORMATS == "cache,sub,buf,dma" == ",".join(gpu.VMEM_CHECKS)
    assert nbc.GPU_PROBE_VMEM_TOKENS == ("vmem",) and nbc.GPU_PROBE_MFMA16_TOKENS == ("mfma16",)
    assert _args(value, env) == want


def test_params_env_carries_the_switch():
    from odh_kubeflow_amd.deploy.manifests import params_env

    assert "GPU_PROBE_MFMA16=false\nGPU_PROBE_VMEM=false\n" in params_env("v0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("manager", "control-plane"):
        with open(os.path.join(root, "config", d, "params.env"), encoding="utf-8") as f:
            assert "GPU_PROBE_VMEM=false\n" in f.read()


@pytest.mark.parametrize("check", list(gpu.VMEM_CHECKS))
def test_fault_counts_of_the_bytes_the_gpu_test_changes(check):
    cases = gpu.vmem_cases(check)
    for byte in (5, 770):
        n = gpu.vmem_fault_count(check, byte)
        assert 0 < n < cases and n % gpu.ODH_VM_BLOCKS == 0, (check, byte, n)
        assert n == gpu.vmem_fault_count(check, byte ^ 3)  # any byte of the key dword
    # every compared element uses exactly one key dword
    assert sum(gpu.vmem_fault_count(check, 4 * k) for k in range(gpu.ODH_VM_TABLE // 4)) == cases
    assert gpu.vmem_fault_count(gpu.ODH_VM_DMA + 1, 5) == 0 and gpu.vmem_fault_count(-1, 5) == 0
    assert gpu.vmem_fault_count("l2", 5) == 0 and gpu.vmem_fault_count(check, gpu.ODH_VM_TABLE) == 0
