"""The C++ mirror (include/mlhip_driver.hpp) of the Gt wire codec, the membership test and Gt.Inverse, through
tests/cpp/gt_codec_test.cpp on a handful of the cases of tests/gt_codec_cases.py: a member, 1, a product; 0, a raw Miller
value, an easy-part output, a flipped bit; two malformed encodings."""
import os
import subprocess

import pytest

from conftest import ROOT
from gt_codec_cases import CURVES, inverse_bytes, wires
from oracle import pyref as R

pytestmark = pytest.mark.gpu

PICKED = ("pairing", "one", "product", "zero", "miller", "easy-part", "bit-flip", "first-coordinate-p", "outside-and-malformed")


def test_cpp_mirror_gt_codec(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "gt_codec_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    so = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    exe = os.path.join(ROOT, "tests", "cpp", "gt_codec_test")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(so)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    lines = []
    for name in CURVES:
        cp = R.CURVES[name]
        inv = inverse_bytes(name)
        for w in wires(name):
            if w.label in PICKED:
                value = R.gt_to_mont_bytes(cp, w.f).hex() if w.f is not None else "-"
                lines.append("%d %s %d %s %s %s" % (cp.curve_id, w.label, w.status, w.wire.hex(), value, inv[w.label].hex() if w.f is not None else "-"))
    path = tmp_path / "gt_codec_cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in CURVES:
        assert "%s gt_codec %d/%d" % (name, len(PICKED), len(PICKED)) in out.stdout
