"""The C++ mirror of the prepared G2 handles (include/mlhip_driver.hpp: G2Prepared) through its test program
tests/cpp/g2_prepared_test.cpp, on the GPU: PairingBatch / MillerLoopBatch equal the Pairing2 + FExp they replace, with and
without an index, on every curve."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "tests", "cpp", "g2_prepared_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "g2_prepared_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    lib = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(lib)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", BIN,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    return BIN


def test_cpp_g2_prepared_mirror():
    co = load_golden("BLS12-377")["g2_gen_coords"]  # the mirror has no built-in BLS12-377 G2 generator
    out = subprocess.run([_build(), co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381", "BLS12-377"):
        assert "%s g2_prepared 7/7 indexed 14/14" % name in out.stdout
