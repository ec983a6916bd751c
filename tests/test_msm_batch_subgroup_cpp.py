"""The C++ mirror (include/mlhip_driver.hpp: MultiScalarMulBatchSubgroup / MultiScalarMulG2BatchSubgroup) and the batched-MSM
functions of the inline header include/mlhip_subgroup.h, compiled as C (tests/cpp/msm_batch_subgroup_c.c) and as C++, through
tests/cpp/msm_batch_subgroup_test.cpp: equal to the plain batch mirrors and to single MultiScalarMul calls on multiples of
the generators on every curve, and the wrappers' argument errors in both languages."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12-381", "BLS12-377")


def test_cpp_mirror_msm_batch_subgroup():
    cpp = os.path.join(ROOT, "tests", "cpp")
    src, csrc = os.path.join(cpp, "msm_batch_subgroup_test.cpp"), os.path.join(cpp, "msm_batch_subgroup_c.c")
    inc = os.path.join(ROOT, "include")
    hdrs = [os.path.join(inc, h) for h in ("mlhip_driver.hpp", "mlhip_subgroup.h", "mlhip.h")]
    so = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    exe, cobj = os.path.join(cpp, "msm_batch_subgroup_test"), os.path.join(cpp, "msm_batch_subgroup_c.o")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src, csrc, so] + hdrs):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", csrc, "-o", cobj])
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", inc, src, cobj, "-o", exe,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    co = load_golden("BLS12-377")["g2_gen_coords"]  # the mirror has no built-in BLS12-377 G2 generator
    out = subprocess.run([exe, co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in CURVES:
        assert "%s MultiScalarMulBatchSubgroup G1 6/6 G2 6/6" % name in out.stdout
