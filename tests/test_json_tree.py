"""The apiserver's copy-on-write JSON tree (``testing/native/apiserver/json.hpp``).

``tests/native/json_tree_check.cpp`` is a stand-alone program (its own ``main``) that includes
the header and checks, at the smallest shapes that can go wrong — objects of 0, 1 and 2
members, three levels deep, an array of objects, keys of 15 and 16 bytes (the last inline key
and the first interned one), strings of 14 and 15 bytes (the last held in the value, the first
behind a payload), every escape and a surrogate pair, a duplicated key, one subtree at two
places of another tree:

* parse then dump gives the input byte for byte, member order kept;
* after a copy, every mutator at every depth leaves the original's dump unchanged and the copy
  holds exactly the edit;
* ``==`` agrees with a node-by-node comparison, for shared and for separately parsed trees;
* once every tree is gone no interned key is left;
* eight threads copy and edit one shared tree while two dump it, and the dumps never change.

It is built and run plain, with AddressSanitizer + UBSan, and with ThreadSanitizer (the
threaded case).  The program is a child process: no sanitizer is loaded into Python.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "json_tree_check.cpp")
INC = os.path.join(ROOT, "odh_kubeflow_amd", "testing", "native", "apiserver")


def _build(tmp, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    out = os.path.join(tmp, "json_tree_check" + ("-" + sanitize.replace(",", "-") if sanitize else ""))
    cmd = ["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror",
           "-I", INC, SRC, "-o", out]
    if sanitize:
        cmd.insert(1, f"-fsanitize={sanitize}")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if sanitize and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip(f"-fsanitize={sanitize} unavailable: {r.stderr[-300:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("sanitize", ["", "address,undefined", "thread"])
def test_json_tree(tmp_path, sanitize):
    binary = _build(str(tmp_path), sanitize)
    env = dict(os.environ)
    env.update({"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1",
                "TSAN_OPTIONS": "halt_on_error=1"})
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert r.stdout.startswith("OK "), report
    for word in ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert word not in r.stderr, report
