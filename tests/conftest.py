import asyncio
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: multi-process or long-running test")


@pytest.fixture
def sock_dir(tmp_path):
    """A directory for unix sockets.  ``sun_path`` holds 107 bytes, and ``tmp_path`` (under
    ``$TMPDIR``, the test name in it) can be longer than that: then a short directory under
    ``/tmp`` is used instead, removed afterwards."""
    if len(os.fsencode(str(tmp_path))) <= 80:
        yield tmp_path
        return
    import pathlib
    import shutil
    import tempfile

    d = tempfile.mkdtemp(prefix="odh-", dir="/tmp")
    try:
        yield pathlib.Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def run():
    """Run a coroutine to completion on a fresh event loop."""
    def _run(coro, timeout=60):
        return asyncio.run(asyncio.wait_for(coro, timeout))
    return _run
