"""The batched MSM without a GPU: the ABI declares and exports mlhip_msm_batch / _device, and the layout builder and
per-lane bodies of mathlib_amd/csrc/msm_batch.h, compiled for the CPU (tests/hostmath_batch), give cref.msm's bytes for
every segment -- every curve, G1 and G2, every compiled chunk length P, segment lengths 0, 1, P - 1, P, P + 1 and 1000, and
the degenerate pairs of tests/msm_batch_cases.py side by side inside one chunk."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from msm_batch_cases import CURVES, curve, edge_segments, expected, point_bytes, random_segments

CHUNKS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def hmb():
    d = os.path.join(ROOT, "tests", "hostmath_batch")
    so = os.path.join(d, "libmsm_batch_host.so")
    src = os.path.join(d, "msm_batch_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hmb_msm_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_size_t,
                                  ctypes.c_int, vp, vp]
    return lib


def offsets_of(lengths):
    offs = (ctypes.c_uint64 * (len(lengths) + 1))()
    for i, m in enumerate(lengths):
        offs[i + 1] = offs[i] + m
    return offs


def run(hmb, cp, group, P, pts, scs, lengths, mont, G=32):
    ps = point_bytes(cp, group)
    out = ctypes.create_string_buffer(max(1, len(lengths)) * ps)
    stats = (ctypes.c_uint64 * 3)()
    rc = hmb.hmb_msm_batch(cp.curve_id, group, P, pts, scs, 1 if mont else 0, offsets_of(lengths), len(lengths), G, out, stats)
    assert rc == 0, rc
    return [out.raw[i * ps : (i + 1) * ps] for i in range(len(lengths))], tuple(stats)


def test_header_declares_and_library_exports_the_batch_entry_points(mlhip):
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    for name in ("mlhip_msm_batch_device", "mlhip_msm_batch"):
        assert re.search(r"^MLHIP_API int %s\(" % name, hdr, re.M), name
    from mathlib_amd import build

    build.build(verbose=False)  # the library as this tree's sources make it
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", os.path.join(ROOT, "mathlib_amd", "libmlhip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if len(ln.split()) >= 3}
    assert {"mlhip_msm_batch_device", "mlhip_msm_batch"} <= exported
    assert "mlhip_msm_batch" in mlhip.SYMBOLS and "mlhip_msm_batch_device" in mlhip.SYMBOLS


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_segments_of_every_length_and_chunk(hmb, name, group):
    cp = curve(name)
    for P in CHUNKS:
        lengths = [0, 1, max(P - 1, 0), P, P + 1, 3, 0, 17, 1000]
        pts, scs, lengths = random_segments(cp, group, lengths, "host/%s/%d/%d" % (name, group, P))
        mont = P in (2, 8)
        got, (chunks, passes, longest) = run(hmb, cp, group, P, pts, scs, lengths, mont)
        assert chunks == sum((m + P - 1) // P for m in lengths)
        assert passes == 2 and longest <= 32  # 1000 pairs: 1000 / P > 32 chunks, summed in two passes
        assert got == expected(cp, group, pts, scs, lengths, mont), (name, group, P)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_degenerate_pairs_inside_one_chunk(hmb, name, group):
    cp = curve(name)
    for pad in (0, 1, 3):
        pts, scs, lengths = edge_segments(cp, group, "host-edge/%s/%d" % (name, group), pad)
        for mont in (False, True):
            exp = expected(cp, group, pts, scs, lengths, mont)
            for P in CHUNKS:
                got, _ = run(hmb, cp, group, P, pts, scs, lengths, mont)
                assert got == exp, (name, group, pad, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])
    # the cancellations really are the point at infinity, and the repeats really doubled: the cases test what they claim
    ps = point_bytes(cp, group)
    pts, scs, lengths = edge_segments(cp, group, "host-edge/%s/%d" % (name, group), 0)
    exp = expected(cp, group, pts, scs, lengths, False)
    for i in (2, 4, 6, 10, 11, 14):
        assert exp[i] == bytes(ps), i
    assert exp[7] != bytes(ps) and exp[16] != bytes(ps)  # [1] P + [r - 1](-P) = 2 P


@pytest.mark.parametrize("P", CHUNKS)
def test_sum_passes_bound_every_lane(hmb, P):
    """Long segments among tiny ones with a small group size: several passes, no group longer than G, same bytes."""
    cp = curve("BLS12-381")
    lengths = [0, 200, 1, 2, 0, 77, 3]
    pts, scs, lengths = random_segments(cp, 1, lengths, "host-passes/%d" % P)
    exp = expected(cp, 1, pts, scs, lengths, False)
    for G in (2, 3, 32):
        got, (chunks, passes, longest) = run(hmb, cp, 1, P, pts, scs, lengths, False, G)
        assert got == exp, (P, G)
        assert longest <= G
        most = -(-200 // P)
        want = 1
        while most > G:
            most, want = -(-most // G), want + 1
        assert passes == want, (P, G)


def test_all_segments_empty(hmb):
    cp = curve("BN254")
    for group in (1, 2):
        got, (chunks, passes, _) = run(hmb, cp, group, 4, b"", b"", [0, 0, 0], False)
        assert chunks == 0 and passes == 1
        assert got == [bytes(point_bytes(cp, group))] * 3
