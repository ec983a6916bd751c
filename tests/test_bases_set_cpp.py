"""The C++ mirror's sets of resident bases (include/mlhip_driver.hpp: BasesG2, BasesSet) and the inline header
include/mlhip_bases_set.h, compiled as C (tests/cpp/bases_set_c.c) and as C++, through tests/cpp/bases_set_test.cpp: every
member's result equals its own MSM, the route is reported, the members outlive the set."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_mirror_bases_set():
    cpp = os.path.join(ROOT, "tests", "cpp")
    src, csrc = os.path.join(cpp, "bases_set_test.cpp"), os.path.join(cpp, "bases_set_c.c")
    inc = os.path.join(ROOT, "include")
    hdrs = [os.path.join(inc, h) for h in ("mlhip_driver.hpp", "mlhip_bases_set.h", "mlhip.h")]
    so = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    exe, cobj = os.path.join(cpp, "bases_set_test"), os.path.join(cpp, "bases_set_c.o")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src, csrc, so] + hdrs):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", csrc, "-o", cobj])
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", inc, src, cobj, "-o", exe,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381"):
        assert "%s BasesSet 6/6" % name in out.stdout
