"""The C++ mirror's short-scalar MSM (include/mlhip_driver.hpp: MultiScalarMulShort, MultiScalarMulG2Short) through its test
program tests/cpp/msm_bits_test.cpp, on the GPU: the bytes the oracle gives for the masked scalars, computed here."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "tests", "cpp", "msm_bits_test")
N, K0, K1, BITS = 48, 12345, 77, 70
M64 = (1 << 64) - 1


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "msm_bits_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    lib = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(lib)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", BIN,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    return BIN


def scalar(i: int) -> int:
    """the program's limbs_of(i): four limbs of one 64-bit multiplicative generator, top nibble cleared, scalar 0 = 0"""
    if i == 0:
        return 0
    x = (0x9E3779B97F4A7C15 * (i + 1)) & M64
    limbs = []
    for _ in range(4):
        x = (x * 6364136223846793005 + 1442695040888963407) & M64
        limbs.append(x)
    limbs[3] &= 0x0FFFFFFFFFFFFFFF
    return sum(l << (64 * k) for k, l in enumerate(limbs))


def test_cpp_msm_bits_mirror():
    from oracle import cref

    masked = b"".join((scalar(i) & ((1 << BITS) - 1)).to_bytes(32, "little") for i in range(N))
    golden = [cref.msm(cid, 1, cref.gen_points(cid, 1, K0, K1, N), masked, N, False, 0, 1).hex() for cid in (0, 1, 2)]
    out = subprocess.run([_build(), str(BITS)] + golden, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381", "BLS12-377"):
        assert "%s short_g1 golden 1 g2 1" % name in out.stdout
