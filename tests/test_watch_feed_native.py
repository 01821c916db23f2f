"""The framer of a watch response body (``native/watch_feed.hpp``), without Python around it.

``tests/native/watch_feed_check.cpp`` is a stand-alone program (its own ``main``) that includes
the header and frames one chunked body whole, byte by byte, cut in two at every offset and cut
in five at 500 seeded random places, then bodies cut short, truncated / oversized / malformed
chunk sizes, a missing CRLF after the chunk data, ``Content-Length`` and EOF-delimited bodies
and a consumer that stops.  Every piece is fed from a buffer of its exact size.

It is built and run plain and with AddressSanitizer + UBSan.  The program is a child process:
no sanitizer is loaded into Python.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "watch_feed_check.cpp")
INC = os.path.join(ROOT, "odh_kubeflow_amd", "native")


def _build(tmp, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    out = os.path.join(tmp, "watch_feed_check" + ("-" + sanitize.replace(",", "-") if sanitize else ""))
    cmd = ["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-Wall", "-Wextra", "-Werror",
           "-I", INC, SRC, "-o", out]
    if sanitize:
        cmd.insert(1, f"-fsanitize={sanitize}")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if sanitize and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip(f"-fsanitize={sanitize} unavailable: {r.stderr[-300:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("sanitize", ["", "address,undefined"])
def test_watch_feed(tmp_path, sanitize):
    binary = _build(str(tmp_path), sanitize)
    env = dict(os.environ)
    env.update({"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"})
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert r.stdout.startswith("OK "), report
    for word in ("AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert word not in r.stderr, report
