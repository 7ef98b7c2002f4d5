"""pytest setup: `gpu` marker, import paths, one-time build of the C libraries."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "daily-ray-trace_amd")
for p in (PKG, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def _make(args):
    r = subprocess.run(["make"] + args, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.fixture(scope="session", autouse=True)
def built_libraries():
    """The .so files are build products, not part of the repo: build what is missing or older than its sources (make's own rules)."""
    _make(["-C", os.path.join(REPO, "oracle"), "all"])
    _make(["-C", PKG, "host"])
    if os.path.exists("/opt/rocm/bin/hipcc"):
        _make(["-C", PKG, "hip"])
    yield


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(REPO, "tests", "golden")
