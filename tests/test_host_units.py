"""Builds and runs the stand-alone tests of the two host headers, each an ordinary executable under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/c/test_host_symbolic.cpp (qpalm_amd/csrc/qpalm_host_symbolic.h: ordering, symbolic factorisation, launch plans)
and tests/c/test_host_convert.cpp (qpalm_amd/csrc/qpalm_host_convert.h: a caller's problem into the device layout, every refusal).
Nothing is loaded into Python.  Sanitizer runs belong on a machine without a GPU: the tests skip themselves where torch sees one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _gpu_visible():
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


@pytest.mark.parametrize("name", ["test_host_symbolic", "test_host_convert"])
def test_host_header_under_sanitizers(name):
    if _gpu_visible():
        pytest.skip("sanitizer runs belong on a machine without a GPU")
    exe = os.path.join(CDIR, name + "_asan")
    r = subprocess.run(["g++"] + FLAGS + ["-o", exe, os.path.join(CDIR, name + ".cpp")], capture_output=True, text=True)
    assert r.returncode == 0, "g++ failed:\n" + r.stderr[-3000:]
    assert not r.stderr.strip(), "the build must be silent under -Wall -Wextra (a warning or note fails this test on purpose):\n" + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "0 failures"
