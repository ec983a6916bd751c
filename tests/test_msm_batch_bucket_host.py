"""The bucket route of the batched MSM without a GPU: the plan, the rows and the per-lane bodies of
mathlib_amd/csrc/msm_batch_bucket.h, compiled for the CPU (tests/hostmath_bucket) and replayed in the kernels' order -- digit
bytes, the 64 lanes of every (slice, window), the lock-step reduction, Horner -- give cref.msm's bytes for every segment of
tests/msm_batch_bucket_cases.py on every curve, with Montgomery and plain scalars; every row of the chunk table belongs to
exactly one kernel kind; an all-short batch keeps the Straus layout byte for byte; and the ABI has not grown."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from msm_batch_bucket_cases import CURVES, FORCED_MIN, FORCED_SLICE, MIXED_LENGTHS, all_ones_scalar, cases, curve
from msm_batch_cases import expected, point_bytes, random_segments

FR_BITS = {"BN254": 254, "BLS12-381": 255, "BLS12-377": 253}


@pytest.fixture(scope="module")
def hbk():
    d = os.path.join(ROOT, "tests", "hostmath_bucket")
    so = os.path.join(d, "libmsm_batch_bucket_host.so")
    src = os.path.join(d, "msm_batch_bucket_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hbk_msm_batch.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_long,
                                  ctypes.c_long, ctypes.c_int, vp, vp]
    lib.hbk_layout_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_long, vp, ctypes.c_size_t, vp]
    lib.hbk_constants.argtypes = [vp]
    return lib


def offsets_of(lengths):
    offs = (ctypes.c_uint64 * (len(lengths) + 1))()
    for i, m in enumerate(lengths):
        offs[i + 1] = offs[i] + m
    return offs


def run(hbk, cp, P, pts, scs, lengths, mont, t_req, s_req, G=32):
    ps = point_bytes(cp, 1)
    out = ctypes.create_string_buffer(max(1, len(lengths)) * ps)
    stats = (ctypes.c_uint64 * 5)()
    rc = hbk.hbk_msm_batch(cp.curve_id, P, pts, scs, 1 if mont else 0, offsets_of(lengths), len(lengths), t_req, s_req, G, out,
                           stats)
    assert rc == 0, rc
    return [out.raw[i * ps : (i + 1) * ps] for i in range(len(lengths))], tuple(stats)


def layout(hbk, lengths, P=4, t_req=-1, s_req=-1, fr_bits=255):
    info = (ctypes.c_uint64 * 5)()
    rc = hbk.hbk_layout_check(fr_bits, P, t_req, s_req, offsets_of(lengths), len(lengths), info)
    assert rc == 0, (rc, lengths, P, t_req, s_req, tuple(info))
    return tuple(info)  # rows, slices, T, S, windows


@pytest.mark.parametrize("name", CURVES)
def test_replayed_cases_match_cref(hbk, name):
    """every case with the route forced (segments from 9 pairs, slices of 16), Montgomery and plain scalars"""
    cp = curve(name)
    ps = point_bytes(cp, 1)
    for case, pts, scs, lengths in cases(name):
        for mont in (False, True):
            exp = expected(cp, 1, pts, scs, lengths, mont)
            got, (rows, slices, T, S, passes) = run(hbk, cp, 4, pts, scs, lengths, mont, FORCED_MIN, FORCED_SLICE)
            assert (T, S) == (FORCED_MIN, FORCED_SLICE)
            assert slices == sum(m // 16 + (1 if m % 16 > 4 else 0) for m in lengths if m >= 9), (case, slices)
            assert got == exp, (name, case, mont, [i for i in range(len(exp)) if got[i] != exp[i]])
        plain = expected(cp, 1, pts, scs, lengths, False)
        if case == "cancelling_pairs":
            assert plain[0] == bytes(ps)
        if case == "only_infinities":
            assert plain[0] == bytes(ps) and plain[1] != bytes(ps)
        if case == "one_pair_70_times":
            assert plain[0] != bytes(ps)
    assert all_ones_scalar(cp) < cp.r


@pytest.mark.parametrize("name", CURVES)
def test_other_chunk_and_slice_lengths(hbk, name):
    """the mixed batch with every compiled chunk length beside slices of 5, 9, 16 and 64 pairs (5 = P + 1 at P = 4: the
    shortest slice), two sum passes forced by a small group, and the route off"""
    cp = curve(name)
    case, pts, scs, lengths = cases(name)[-1]
    assert case == "mixed" and lengths == MIXED_LENGTHS
    exp = expected(cp, 1, pts, scs, lengths, False)
    for P, S, G in ((1, 9, 32), (2, 64, 32), (4, 5, 32), (8, 16, 3), (4, 1, 32)):
        got, (rows, slices, T, s_used, passes) = run(hbk, cp, P, pts, scs, lengths, False, 3, S, G)  # 3 means 9
        assert T == 9 and s_used == max(S, P + 1) and slices >= 4, (P, S)
        assert got == exp, (name, P, S, G)
    got, (rows, slices, T, _, _) = run(hbk, cp, 4, pts, scs, lengths, False, 0, 16)
    assert got == exp and slices == 0 and T == 0 and rows == sum(-(-m // 4) for m in lengths)


def test_two_torsion_point_is_what_it_claims():
    from oracle import pyref as R

    cp = curve("BLS12-377")
    p = (cp.p - 1, 0)
    assert R.g1_is_on_curve(cp, p) and R.g1_add(cp, p, p) is None and R.g1_neg(cp, p) == p


def test_rows_around_the_thresholds(hbk):
    """segments of T - 1, T, T + 1, S, S + 1 and 2 S + 1 pairs: below T Straus chunks, from T on slices; the checks of
    hbk_layout_check hold for each alone and for all of them in one batch between empty and short segments"""
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
    (hbk_layout_check compares them), whatever the switches say"""
    lengths = [0, 1, 3, 4, 5, 8, 0, 7, 2000, 33]
    tiny = [0, 1, 3, 4, 5, 8, 0, 7, 8, 2]  # below 9 pairs: short under every setting, the default included
    for P in (1, 2, 4, 8):
        for t_req, s_req in ((0, -1), (0, 16), (2001, 16), (2001, -1), (1 << 40, 7)):
            rows, slices, T, _, _ = layout(hbk, lengths, P, t_req, s_req)
            assert slices == 0 and rows == sum(-(-m // P) for m in lengths), (P, t_req, s_req)
        for t_req, s_req in ((-1, -1), (-1, 16), (1, -1), (9, 5)):
            rows, slices, T, _, _ = layout(hbk, tiny, P, t_req, s_req)
            assert slices == 0 and rows == sum(-(-m // P) for m in tiny), (P, t_req, s_req)
    rows, slices, T, S, _ = layout(hbk, lengths, 4, 2000, 16)
    assert slices == 125 and rows == 125 + sum(-(-m // 4) for m in lengths if m != 2000)


def test_plan(hbk):
    """the switches: MIN 1 .. 8 mean 9, 0 means never, unset means the compiled default; a fixed slice is at least P + 1; the
    plan's own slice length is a power of two between the bounds, grows with the batch and never leaves fewer (slice, window)
    waves than the target while a shorter slice would give more"""
    c = (ctypes.c_uint64 * 4)()
    hbk.hbk_constants(c)
    t_default, s_min, s_max, waves = tuple(c)
    assert t_default == 0 or (t_default >= 9 and t_default & (t_default - 1) == 0)
    assert s_min == 256 and s_max >= s_min and s_max & (s_max - 1) == 0
    for name, bits in FR_BITS.items():
        assert layout(hbk, [100], fr_bits=bits, t_req=9)[4] == 37, name  # 7-bit windows of FR_BITS + 1 bits
    for t_req in range(1, 9):
        assert layout(hbk, [100], t_req=t_req)[2] == 9
    assert layout(hbk, [100], t_req=0)[2] == 0 and layout(hbk, [100])[2] == t_default
    assert layout(hbk, [100], P=8, t_req=9, s_req=3)[3] == 9 and layout(hbk, [100], P=4, t_req=9, s_req=3)[3] == 5
    seen = []
    for lengths in ([5000], [1 << 14] * 4, [1 << 12] * 64, [1 << 16] * 16, [1 << 20], [700] * 1500):
        rows, slices, T, S, W = layout(hbk, lengths, t_req=512)
        assert s_min <= S <= s_max and S & (S - 1) == 0
        assert S == s_min or slices * W >= waves, (lengths[:2], S, slices)
        if S < s_max:
            assert sum(-(-m // (2 * S)) for m in lengths) * W < waves, (lengths[:2], S)
        seen.append(S)
    assert seen[0] == s_min and seen[4] == s_max


def test_header_names_the_switches_and_the_abi_has_not_grown(mlhip):
    from mathlib_amd import build

    fns = build.abi_functions()
    assert len(fns) == 77 and sorted(fns) == sorted(mlhip.SYMBOLS)
    assert "mlhip_msm_batch" in fns and "mlhip_msm_batch_device" in fns
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert "MLHIP_MSM_BATCH_BUCKET_MIN" in hdr and "MLHIP_MSM_BATCH_BUCKET_SLICE" in hdr
    kern = open(os.path.join(ROOT, "mathlib_amd", "csrc", "msm_kernels.h")).read()
    assert kern.index('#include "msm_batch.h"') < kern.index('#include "msm_batch_bucket.h"')
