"""Builds and runs tests/c/test_update_Q_A.c: qpalm_update_Q_A of include/qpalm_host.h (the plain-C host layer) on the golden basic_qp, against a
qpalm_setup on the updated data.  Everything generated goes to the test's temporary directory."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def _emit_header(golden, path):
    p = golden["problems"]["basic_qp"]
    out = ["/* generated from tests/golden/reference_tests.json by tests/test_update_Q_A_host_c.py */", "#include <stddef.h>", "#include <stdint.h>",
           "typedef struct { size_t n, m, nnzA, nnzQ; const int64_t *Ap, *Ai, *Qp, *Qi; const double *Ax, *Qx, *q, *bmin, *bmax; } golden_problem;"]
    for k in ("Ap", "Ai", "Qp", "Qi"):
        out.append("static const int64_t basic_qp_%s[] = {%s};" % (k, ", ".join(str(int(x)) for x in p[k])))
    for k in ("Ax", "Qx", "q", "bmin", "bmax"):
        out.append("static const double basic_qp_%s[] = {%s};" % (k, ", ".join(repr(float(x)) for x in p[k])))
    out.append("static const golden_problem golden_basic_qp = {%d, %d, %d, %d, %s};"
               % (p["n"], p["m"], len(p["Ax"]), len(p["Qx"]), ", ".join("basic_qp_" + k for k in ("Ap", "Ai", "Qp", "Qi", "Ax", "Qx", "q", "bmin", "bmax"))))
    out.append("static const double basic_qp_solution[] = {%s};" % ", ".join(repr(float(x)) for x in golden["expect"]["basic_qp"]["solution"]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def _build_and_run(tmp, libdir, backend_lib, golden):
    tmp = str(tmp)
    _emit_header(golden, os.path.join(tmp, "golden_data.h"))
    host = os.path.join(tmp, "libqpalm_host_under_test.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-fPIC", "-shared", "-Wall", "-Werror", "-o", host,
                           os.path.join(ROOT, "qpalm_amd", "host", "qpalm_host.c"), os.path.join(ROOT, "qpalm_amd", "host", "qpalm_qps.c"),
                           "-L" + libdir, "-l" + backend_lib, "-Wl,-rpath," + libdir, "-lm"])
    exe = os.path.join(tmp, "test_update_Q_A")
    src = os.path.join(tmp, "test_update_Q_A.c")      # a copy next to the generated header: the source includes it by its plain name
    with open(os.path.join(CDIR, "test_update_Q_A.c")) as f:
        text = f.read().replace('"../../include/qpalm_host.h"', '"%s"' % os.path.join(ROOT, "include", "qpalm_host.h"))
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(["gcc", "-O1", "-std=c99", "-Wall", "-o", exe, src, host, "-Wl,-rpath," + tmp, "-Wl,-rpath," + libdir, "-L" + libdir, "-l" + backend_lib, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failures" in r.stdout


def test_update_Q_A_on_emulated_kernels(golden, emu_lib, tmp_path):
    _build_and_run(tmp_path, os.path.dirname(emu_lib), "qpalm_gfx950_emu", golden)


@pytest.mark.gpu
def test_update_Q_A_on_gfx950(golden, tmp_path):
    from qpalm_amd import build
    _build_and_run(tmp_path, os.path.dirname(build.LIB), "qpalm_gfx950", golden)
