"""The G2 bucket route of the batched MSM, and the indexed point load of the table-free path of mlhip_bases_msm_batch*,
without a GPU: the plan, the rows and the per-lane bodies of mathlib_amd/csrc/msm_batch_bucket.h, compiled for the CPU
(tests/hostmath_bucket_g2) and replayed in the kernels' order -- digit bytes lane by lane, the 32 lanes (lane pairs on the
device) of every (slice, window), the ten lock-step reduction steps, Horner, the other rows through msm_batch_chunk, the sum
passes -- give cref.msm's bytes for every segment of tests/msm_batch_bucket_g2_cases.py on every curve, with Montgomery and
plain scalars; 43 windows of magnitudes up to 32; every row of the chunk table belongs to exactly one kernel kind; an
all-short batch keeps the Straus layout byte for byte; the same replay through a base-index list, and through base0
offsets, over 24 bases equals cref on the gathered points (G1 and G2); and the ABI has not grown."""
import ctypes
import os
import random
import subprocess

import pytest

from bases_batch_cases import expected_indexed, gen_bases, positional_index
from conftest import ROOT
from msm_batch_bucket_g2_cases import CURVES, FORCED_MIN, FORCED_SLICE, MIXED_LENGTHS, all_ones_scalar, cases, curve
from msm_batch_cases import expected, point_bytes, sc

FR_BITS = {"BN254": 254, "BLS12-381": 255, "BLS12-377": 253}
DIRECT, INDEXED, POSITIONAL = 0, 1, 2


@pytest.fixture(scope="module")
def hbk():
    d = os.path.join(ROOT, "tests", "hostmath_bucket_g2")
    so = os.path.join(d, "libmsm_batch_bucket_g2_host.so")
    src = os.path.join(d, "msm_batch_bucket_g2_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hbk2_msm_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp, ctypes.c_int, vp,
                                   ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_long, ctypes.c_long, ctypes.c_int, vp, vp]
    lib.hbk2_layout_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_long, vp, ctypes.c_size_t,
                                      vp]
    lib.hbk2_constants.argtypes = [ctypes.c_int, vp]
    return lib


def offsets_of(lengths):
    offs = (ctypes.c_uint64 * (len(lengths) + 1))()
    for i, m in enumerate(lengths):
        offs[i + 1] = offs[i] + m
    return offs


def run(hbk, cp, group, P, pts, scs, lengths, mont, t_req, s_req, G=32, index=None, mode=DIRECT):
    ps = point_bytes(cp, group)
    out = ctypes.create_string_buffer(max(1, len(lengths)) * ps)
    stats = (ctypes.c_uint64 * 6)()
    idx = (ctypes.c_uint32 * max(1, len(index)))(*index) if index is not None else None
    rc = hbk.hbk2_msm_batch(cp.curve_id, group, P, pts, len(pts) // ps, idx, mode, scs, 1 if mont else 0, offsets_of(lengths),
                            len(lengths), t_req, s_req, G, out, stats)
    assert rc == 0, rc
    return [out.raw[i * ps : (i + 1) * ps] for i in range(len(lengths))], tuple(stats)


def layout(hbk, lengths, P=4, t_req=-1, s_req=-1, fr_bits=255, group=2):
    info = (ctypes.c_uint64 * 5)()
    rc = hbk.hbk2_layout_check(fr_bits, group, P, t_req, s_req, offsets_of(lengths), len(lengths), info)
    assert rc == 0, (rc, lengths, P, t_req, s_req, tuple(info))
    return tuple(info)  # rows, slices, T, S, windows


def constants(hbk, group):
    c = (ctypes.c_uint64 * 7)()
    hbk.hbk2_constants(group, c)
    return tuple(c)  # MIN default, SLICE_MIN, SLICE_MAX, waves, width, buckets, reduction steps


@pytest.mark.parametrize("name", CURVES)
def test_replayed_cases_match_cref(hbk, name):
    """every G2 case with the route forced (segments from 9 pairs, slices of 16), Montgomery and plain scalars"""
    cp = curve(name)
    ps = point_bytes(cp, 2)
    seen_largest = 0
    for case, pts, scs, lengths in cases(name):
        for mont in (False, True):
            exp = expected(cp, 2, pts, scs, lengths, mont)
            got, (rows, slices, T, S, passes, largest) = run(hbk, cp, 2, 4, pts, scs, lengths, mont, FORCED_MIN, FORCED_SLICE)
            assert (T, S) == (FORCED_MIN, FORCED_SLICE)
            assert slices == sum(m // 16 + (1 if m % 16 > 4 else 0) for m in lengths if m >= 9), (case, slices)
            assert largest <= 32, (case, largest)
            seen_largest = max(seen_largest, largest)
            assert got == exp, (name, case, mont, [i for i in range(len(exp)) if got[i] != exp[i]])
        plain = expected(cp, 2, pts, scs, lengths, False)
        if case == "cancelling_pairs":
            assert plain[0] == bytes(ps)
        if case == "only_infinities":
            assert plain[0] == bytes(ps) and plain[1] != bytes(ps)
        if case == "one_pair_40_times":
            assert plain[0] != bytes(ps)
    assert seen_largest == 32  # the scalar 32: the last lane pair's bucket is reached
    assert all_ones_scalar(cp) < cp.r


@pytest.mark.parametrize("name", CURVES)
def test_other_chunk_and_slice_lengths(hbk, name):
    """the first seven segments of the mixed batch (0, 40, 3, 0, 17, 9, 8 pairs) with every compiled chunk length P beside
    slices of 5, 9, 16 and 64 pairs (a slice is raised to P + 1), two sum passes forced by groups of 3, and the route off"""
    cp = curve(name)
    case, pts, scs, lengths = cases(name)[-1]
    assert case == "mixed" and lengths == MIXED_LENGTHS
    lengths = lengths[:7]
    n = sum(lengths)
    pts, scs = pts[: n * point_bytes(cp, 2)], scs[: 32 * n]
    exp = expected(cp, 2, pts, scs, lengths, False)
    for P in (1, 2, 4, 8):
        for S in (5, 9, 16, 64):
            got, (rows, slices, T, s_used, passes, _) = run(hbk, cp, 2, P, pts, scs, lengths, False, 3, S)  # 3 means 9
            assert T == 9 and s_used == max(S, P + 1) and slices >= 3, (P, S)
            assert got == exp, (name, P, S)
    got, (_, _, _, _, passes, _) = run(hbk, cp, 2, 4, pts, scs, lengths, False, 9, 5, G=3)
    assert got == exp and passes == 2  # 40 pairs = 8 rows -> 3 partials -> 1: two sum passes
    got, (rows, slices, T, _, _, _) = run(hbk, cp, 2, 4, pts, scs, lengths, False, 0, 16)
    assert got == exp and slices == 0 and T == 0 and rows == sum(-(-m // 4) for m in lengths)


def test_rows_around_the_thresholds(hbk):
    """segments of T - 1, T, T + 1, S, S + 1 and 2 S + 1 pairs: below T Straus chunks, from T on slices"""
    for P in (1, 2, 4, 8):
        for T, S in ((9, 16), (9, 9), (20, 16), (64, 256), (1000, 256)):
            around = [T - 1, T, T + 1, S, S + 1, 2 * S + 1]
            for m in around:
                rows, slices, t_used, s_used, _ = layout(hbk, [m], P, T, S)
                assert (t_used, s_used) == (T, S)
                if m < T:
                    assert slices == 0 and rows == -(-m // P), (P, T, S, m)
                else:
                    assert rows == -(-m // S), (P, T, S, m)
                    assert slices == m // S + (1 if m % S > P else 0), (P, T, S, m)
            rows, slices, _, _, _ = layout(hbk, [0, 3] + around + [0, 1, P, 0], P, T, S)
            assert slices == sum(m // S + (1 if m % S > P else 0) for m in around if m >= T)


def test_all_short_batch_keeps_the_straus_layout(hbk):
    """no segment reaches T (or the route is off): chunk table, groups and passes equal msm_batch_layout's byte for byte
    (hbk2_layout_check compares them), whatever the switches say"""
    lengths = [0, 1, 3, 4, 5, 8, 0, 7, 2000, 33]
    tiny = [0, 1, 3, 4, 5, 8, 0, 7, 8, 2]  # below 9 pairs: short under every setting, the default included
    for group in (1, 2):
        for P in (1, 2, 4, 8):
            for t_req, s_req in ((0, -1), (0, 16), (2001, 16), (2001, -1), (1 << 40, 7)):
                rows, slices, T, _, _ = layout(hbk, lengths, P, t_req, s_req, group=group)
                assert slices == 0 and rows == sum(-(-m // P) for m in lengths), (P, t_req, s_req)
            for t_req, s_req in ((-1, -1), (-1, 16), (1, -1), (9, 5)):
                rows, slices, T, _, _ = layout(hbk, tiny, P, t_req, s_req, group=group)
                assert slices == 0 and rows == sum(-(-m // P) for m in tiny), (P, t_req, s_req)
    rows, slices, T, S, _ = layout(hbk, lengths, 4, 2000, 16)
    assert slices == 125 and rows == 125 + sum(-(-m // 4) for m in lengths if m != 2000)


def test_geometry_and_plan(hbk):
    """G2: 6-bit windows, 43 of them on every curve, 32 buckets, ten reduction steps; G1 is what it was.  The switches mean
    the same in both groups; the defaults are the group's own; the plan's own slice length is a power of two between the
    group's bounds and never leaves fewer (slice, window) waves than the target while a shorter slice would give more."""
    t1, s1_min, s1_max, waves1, width1, buckets1, steps1 = constants(hbk, 1)
    assert (t1, s1_min, s1_max, waves1, width1, buckets1, steps1) == (512, 256, 4096, 4096, 7, 64, 12)
    t2, s_min, s_max, waves, width, buckets, steps = constants(hbk, 2)
    assert (width, buckets, steps) == (6, 32, 10)
    assert t2 == 0 or (t2 >= 9 and t2 & (t2 - 1) == 0)
    assert s_min > 8 and s_max >= s_min and s_min & (s_min - 1) == 0 and s_max & (s_max - 1) == 0 and waves > 0
    for name, bits in FR_BITS.items():
        assert layout(hbk, [100], fr_bits=bits, t_req=9)[4] == 43, name
        assert layout(hbk, [100], fr_bits=bits, t_req=9, group=1)[4] == 37, name
    for t_req in range(1, 9):
        assert layout(hbk, [100], t_req=t_req)[2] == 9
    assert layout(hbk, [100], t_req=0)[2] == 0
    assert layout(hbk, [100])[2] == t2 and layout(hbk, [100], group=1)[2] == t1
    assert layout(hbk, [100], P=8, t_req=9, s_req=3)[3] == 9 and layout(hbk, [100], P=4, t_req=9, s_req=3)[3] == 5
    for lengths in ([5000], [1 << 14] * 4, [1 << 12] * 64, [1 << 16] * 16, [1 << 20], [700] * 1500):
        rows, slices, T, S, W = layout(hbk, lengths, t_req=512)
        assert s_min <= S <= s_max and S & (S - 1) == 0
        assert S == s_min or slices * W >= waves, (lengths[:2], S, slices)
        if S < s_max:
            assert sum(-(-m // (2 * S)) for m in lengths) * W < waves, (lengths[:2], S)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_indexed_loader_over_24_bases(hbk, name, group):
    """the table-free path of mlhip_bases_msm_batch*: the replay reads pair j of a row through the index list (repeats, one
    base many times, a base at infinity), or at base0 + j without one, over a table of 24 bases"""
    cp = curve(name)
    ps = point_bytes(cp, group)
    rnd = random.Random("bucket-bases-host/%s/%d" % (name, group))
    bases = bytearray(gen_bases(cp, group, 24, 7))
    bases[5 * ps : 6 * ps] = bytes(ps)  # base 5: the point at infinity
    bases = bytes(bases)
    lengths = [0, 40, 3, 17, 9, 70]
    index = [rnd.randrange(24) for _ in range(sum(lengths))]
    index[43:60] = [11] * 17  # the segment of 17 pairs: one base all the way
    index[4] = index[20] = index[69] = index[138] = 5
    scs = b"".join(sc(rnd.getrandbits(256)) for _ in range(sum(lengths)))
    for mont in (False, True):
        exp = expected_indexed(cp, group, bases, index, scs, lengths, mont)
        for t_req in (FORCED_MIN, 0):
            got, (rows, slices, _, _, _, _) = run(hbk, cp, group, 4, bases, scs, lengths, mont, t_req, FORCED_SLICE, index=index,
                                                  mode=INDEXED)
            assert got == exp and (slices > 0) == (t_req > 0), (name, group, mont, t_req)
    short = [0, 24, 3, 17, 9, 20]  # without a list a segment reads bases 0 .. m - 1: at most 24 pairs
    scs = scs[: 32 * sum(short)]
    exp = expected_indexed(cp, group, bases, positional_index(short), scs, short, False)
    for t_req in (FORCED_MIN, 0):
        got, (rows, slices, _, _, _, _) = run(hbk, cp, group, 4, bases, scs, short, False, t_req, FORCED_SLICE, mode=POSITIONAL)
        assert got == exp and (slices > 0) == (t_req > 0), (name, group, t_req)


def test_header_names_the_switches_and_the_abi_has_not_grown(mlhip):
    from mathlib_amd import build

    fns = build.abi_functions()
    assert len(fns) == 77 and sorted(fns) == sorted(mlhip.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert "MLHIP_MSM_BATCH_BUCKET_MIN" in hdr and "MLHIP_MSM_BATCH_BUCKET_SLICE" in hdr
    kern = open(os.path.join(ROOT, "mathlib_amd", "csrc", "msm_kernels.h")).read()
    assert kern.index('#include "msm_batch_bucket.h"') < kern.index('#include "msm_bases_batch.h"')
