"""The C++ mirror's products of any length (include/mlhip_driver.hpp: Curve::MillerLoopProducts / PairingProducts and
G2Prepared with more than four pairs per product, over include/mlhip_products.h) through its test program
tests/cpp/pairing_products_test.cpp, on the GPU: one case per curve against PairingProduct on each product."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "tests", "cpp", "pairing_products_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "pairing_products_test.cpp")
    hdrs = [os.path.join(ROOT, "include", h) for h in ("mlhip_driver.hpp", "mlhip_products.h", "mlhip.h")]
    lib = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in [src, lib] + hdrs):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", BIN,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    return BIN


def test_cpp_pairing_products_mirror():
    co = load_golden("BLS12-377")["g2_gen_coords"]  # the mirror has no built-in BLS12-377 G2 generator
    out = subprocess.run([_build(), co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381", "BLS12-377"):
        assert "%s products 3/3 prepared 3/3" % name in out.stdout
