"""The batched MSM over resident bases without a GPU: the ABI declares and exports mlhip_bases_msm_batch / _device /
mlhip_bases_batch_tabled, and the per-lane body of mathlib_amd/csrc/msm_bases_batch.h, compiled for the CPU
(tests/hostmath_bases_batch) over per-base tables computed on the host, gives cref.msm's bytes for every segment -- every
curve, G1 and G2, several table widths w, every chunk length P, with and without an index list, repeated indices, and the
degenerate segments of tests/msm_batch_cases.py (bases at infinity, the accumulator meeting +-its own table entry)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from bases_batch_cases import edge_indexed, expected_indexed, gen_bases, positional_index, random_indexed
from conftest import ROOT
from msm_batch_cases import CURVES, curve, expected, point_bytes, random_segments

CHUNKS = (1, 2, 4, 8, 16)
NEW = ("mlhip_bases_msm_batch", "mlhip_bases_msm_batch_device", "mlhip_bases_batch_tabled")


@pytest.fixture(scope="module")
def hbb():
    d = os.path.join(ROOT, "tests", "hostmath_bases_batch")
    so = os.path.join(d, "libbases_batch_host.so")
    src = os.path.join(d, "bases_batch_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hbb_bases_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp, ctypes.c_int,
                                    vp, vp, ctypes.c_size_t, vp, vp]
    return lib


def run(hbb, cp, group, w, P, bases, scs, lengths, mont, index=None):
    ps = point_bytes(cp, group)
    n = len(bases) // ps
    offs = (ctypes.c_uint64 * (len(lengths) + 1))()
    for i, m in enumerate(lengths):
        offs[i + 1] = offs[i] + m
    idx = None if index is None else (ctypes.c_uint32 * max(1, len(index)))(*index)
    out = ctypes.create_string_buffer(max(1, len(lengths)) * ps)
    stats = (ctypes.c_uint64 * 2)()
    rc = hbb.hbb_bases_batch(cp.curve_id, group, w, P, bases, n, scs, 1 if mont else 0, idx, offs, len(lengths), out, stats)
    assert rc == 0, rc
    return [out.raw[i * ps : (i + 1) * ps] for i in range(len(lengths))], tuple(stats)


def test_header_declares_and_library_exports_the_bases_batch_entry_points(mlhip):
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    for name in NEW:
        assert re.search(r"^MLHIP_API int %s\(" % name, hdr, re.M), name
    from mathlib_amd import build

    assert set(NEW) <= set(build.abi_functions())
    assert set(NEW) <= set(mlhip.SYMBOLS)
    build.build(verbose=False)  # the library as this tree's sources make it
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", os.path.join(ROOT, "mathlib_amd", "libmlhip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if len(ln.split()) >= 3}
    assert set(NEW) <= exported


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_indexed_segments_every_width_and_chunk(hbb, name, group):
    cp = curve(name)
    n = 6
    bases = gen_bases(cp, group, n, 1)
    for w in (4, 5, 7):
        for P in CHUNKS:
            lengths = [0, 1, max(P - 1, 0), P, P + 1, 3, 0, 2 * P + 3]
            index, scs = random_indexed(cp, n, lengths, "host/%s/%d/%d/%d" % (name, group, w, P))
            mont = P in (2, 8)
            got, (chunks, _) = run(hbb, cp, group, w, P, bases, scs, lengths, mont, index)
            assert chunks == sum((m + P - 1) // P for m in lengths)
            assert got == expected_indexed(cp, group, bases, index, scs, lengths, mont), (name, group, w, P)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_positional_segments_of_every_length(hbb, name, group):
    """no index list: pair j of every segment takes base j, segments of every length 0 .. n in random order"""
    cp = curve(name)
    n = 9
    bases = gen_bases(cp, group, n, 2)
    lengths = [9, 0, 4, 1, 8, 2, 7, 3, 6, 5, 9]
    _, scs, _ = random_segments(cp, group, lengths, "host-pos/%s/%d" % (name, group))
    index = positional_index(lengths)
    for w, P in ((6, 4), (8, 16), (4, 1)):
        got, _ = run(hbb, cp, group, w, P, bases, scs, lengths, False, None)
        assert got == expected_indexed(cp, group, bases, index, scs, lengths, False), (name, group, w, P)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_degenerate_segments(hbb, name, group):
    """bases at infinity, zero scalars, scalars >= r, the same base twice, (B, s) beside (-B, s) and (B, r - s), inside
    one chunk and across chunk boundaries"""
    cp = curve(name)
    for pad in (0, 1, 3):
        bases, index, scs, lengths = edge_indexed(cp, group, "host-edge/%s/%d" % (name, group), pad)
        for mont in (False, True):
            exp = expected_indexed(cp, group, bases, index, scs, lengths, mont)
            for w, P in ((4, 1), (4, 4), (5, 16), (6, 8), (8, 2)):
                got, _ = run(hbb, cp, group, w, P, bases, scs, lengths, mont, index)
                assert got == exp, (name, group, pad, mont, w, P, [i for i in range(len(exp)) if got[i] != exp[i]])


def test_one_base_repeated(hbb):
    """every pair of a segment on base 0: [1]B + [1]B + ... and [s]B + [r - s]B through the exact path of the mixed addition"""
    cp = curve("BLS12-381")
    r = cp.r
    bases = gen_bases(cp, 1, 3, 3)
    vals = [[1, 1], [1, 1, 1, 1], [5, r - 5], [7, r - 7, 7], [r - 1, 1, 2], [(1 << 256) - 1, 1]]
    lengths = [len(v) for v in vals]
    scs = b"".join(x.to_bytes(32, "little") for v in vals for x in v)
    index = [0] * sum(lengths)
    exp = expected_indexed(cp, 1, bases, index, scs, lengths, False)
    assert exp[2] == bytes(96) and exp[0] != bytes(96)
    for w in (4, 8):
        for P in CHUNKS:
            got, _ = run(hbb, cp, 1, w, P, bases, scs, lengths, False, index)
            assert got == exp, (w, P)


def test_all_segments_empty(hbb):
    cp = curve("BN254")
    for group in (1, 2):
        bases = gen_bases(cp, group, 2, 4)
        got, (chunks, passes) = run(hbb, cp, group, 4, 8, bases, b"", [0, 0, 0], False, [])
        assert chunks == 0 and passes == 1
        assert got == [bytes(point_bytes(cp, group))] * 3
        assert expected(cp, group, b"", b"", [0], False) == [bytes(point_bytes(cp, group))]
