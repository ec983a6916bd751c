"""The C++ mirror's batched MSM (include/mlhip_driver.hpp: MultiScalarMulBatch, MultiScalarMulG2Batch, Mul2Batch) through
its test program tests/cpp/msm_batch_test.cpp, on the GPU: every segment equals the single MSM it batches."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "tests", "cpp", "msm_batch_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "msm_batch_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    lib = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(lib)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", BIN,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    return BIN


def test_cpp_msm_batch_mirror():
    co = load_golden("BLS12-377")["g2_gen_coords"]
    out = subprocess.run([_build(), co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381", "BLS12-377"):
        assert "%s msm_batch_g1 6/6 mul2_batch 8/8" % name in out.stdout
        assert "%s msm_batch_g2 4/4" % name in out.stdout
