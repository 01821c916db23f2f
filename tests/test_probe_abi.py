"""The probe library's C ABI (``csrc/gpu_probe.h``) against its ctypes mirror in ``ops/gpu.py``.

Reads the header and the two sources as text: no library is loaded and no GPU is needed.
"""

import os
import re

from odh_kubeflow_amd.ops import gpu

CSRC = os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc")


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _code(text):
    """``text`` without comments."""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def _header():
    """(functions: name -> parameter count, constants: name -> value) declared by the header."""
    code = _code(_read("gpu_probe.h"))
    block = re.search(r'extern\s+"C"\s*\{(.*)\}', code, re.S).group(1)
    functions = {}
    for decl in block.split(";"):
        m = re.match(r"\s*[\w\s\*]+?\b(odh_\w+)\s*\((.*)\)\s*$", decl, re.S)
        if m:
            params = m.group(2).strip()
            functions[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    constants = {k: int(v, 0) for k, v in re.findall(r"\b(ODH_\w+)\s*=\s*(\w+)\s*,", code)}
    return functions, constants


FUNCTIONS, CONSTANTS = _header()


def test_header_parses():
    assert len(FUNCTIONS) >= 20 and FUNCTIONS["odh_probe_preload"] == 0 and FUNCTIONS["odh_probe_cli"] == 2
    assert FUNCTIONS["odh_probe_graph_create"] == 13
    assert CONSTANTS["ODH_NCOUNT"] == 32 and len(CONSTANTS) >= 10


def test_signature_table_matches_header():
    for name, (_restype, argtypes) in gpu.SIGNATURES.items():
        assert name in FUNCTIONS, f"{name} is not declared in gpu_probe.h"
        assert len(argtypes) == FUNCTIONS[name], f"{name}: {len(argtypes)} argtypes, {FUNCTIONS[name]} parameters"


def test_slot_constants_match_header():
    mirrored = {k: v for k, v in vars(gpu).items() if k.startswith("ODH_")}
    assert mirrored == CONSTANTS


def test_every_declared_function_is_defined():
    sources = _code(_read("gpu_probe.hip")) + _code(_read("probe_cli.cpp"))
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\([^;{]*\)\s*\{" % name, sources), f"{name} is declared but not defined"
