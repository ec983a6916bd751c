"""The C++ mirror's batched MSM over resident bases (include/mlhip_driver.hpp: Bases::MultiScalarMulBatch) through its test
program tests/cpp/bases_batch_test.cpp, on the GPU: every segment equals the MSM it batches, with and without index lists."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "tests", "cpp", "bases_batch_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "bases_batch_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    lib = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(lib)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", BIN,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    return BIN


def test_cpp_bases_batch_mirror():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381", "BLS12-377"):
        assert "%s bases_batch 4/4 indexed 4/4" % name in out.stdout
