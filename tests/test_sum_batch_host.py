"""The segmented point sums (the batch calls with MLHIP_SCALARS_UNIT) without a GPU: the slice layout, the choice of S and
the slice body of mathlib_amd/csrc/msm_sum_batch.h, compiled for the CPU (tests/hostmath_sum_batch), give oracle.pyref's sum
for every segment of tests/sum_batch_cases.py on every curve and group at S = 1, 4 and the default; the slice tables read
every point index of every segment exactly once and no chain exceeds max(S, 32); the S rule stays within its bounds; the real
library checks the flagged calls' arguments before it asks for a device; the three drivers have the methods and the C ABI
has not grown."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from point_sum_cases import CURVES
from sum_batch_cases import LENGTHS, TOTAL, batch, curve, indexed_batch, offsets_of, point_bytes

MAX_LANES = {1: 65536, 2: 32768}
UNIT = 0x400


@pytest.fixture(scope="module")
def hsb():
    d = os.path.join(ROOT, "tests", "hostmath_sum_batch")
    so = os.path.join(d, "libsum_batch_host.so")
    src = os.path.join(d, "sum_batch_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hsb_sum_batch.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_uint32, vp, vp]
    lib.hsb_layout_check.argtypes = [vp, ctypes.c_size_t, ctypes.c_uint32, vp]
    lib.hsb_slice_default.argtypes = [ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int]
    lib.hsb_slice_default.restype = ctypes.c_uint32
    lib.hsb_slice_valid.argtypes = [ctypes.c_long]
    return lib


def c_offsets(lengths):
    o = offsets_of(lengths)
    return (ctypes.c_uint64 * len(o))(*o)


def replay(hsb, cp, group, raw, lengths, S, mode=0, index=None):
    ps = point_bytes(cp, group)
    out = ctypes.create_string_buffer(ps * len(lengths))
    stats = (ctypes.c_uint64 * 3)()
    idx = None if index is None else (ctypes.c_uint32 * max(1, len(index)))(*index)
    rc = hsb.hsb_sum_batch(cp.curve_id, group, raw, mode, idx, c_offsets(lengths), len(lengths), S, out, stats)
    assert rc == 0, rc
    return [out.raw[i * ps : (i + 1) * ps] for i in range(len(lengths))], tuple(stats)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_replayed_sums_match_pyref(hsb, name, group):
    """every segment of the batch at S = 1 (one slice per point: the sum passes do all the work), S = 4 (129 points need a
    middle pass) and the default rule (4 for a call this small)"""
    cp = curve(name)
    raw, exp = batch(name, group)
    ps = point_bytes(cp, group)
    for S in (1, 4, 0):
        got, (s_used, slices, passes) = replay(hsb, cp, group, raw, LENGTHS, S)
        assert got == list(exp), (name, group, S)
        assert s_used == (S or 4)
        assert slices == sum(-(-m // s_used) for m in LENGTHS)
        assert passes == 2  # S = 1: 129 slices in 5 groups, then 1; S = 4: 33 slices in 2 groups, then 1
    # the cases test what they claim: empty, all-infinity, pairs of even length and sums-to-infinity segments are infinity
    zero = bytes(ps)
    assert [e == zero for e in exp] == [True, False, True, True, False, True, False, True, False, False, True]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_replayed_handle_loads_match_pyref(hsb, name, group):
    """the two loads of the handle forms: bases[base_index[i]] (repeats, a base in two segments, an empty list) and
    bases[i - a], at S = 1, 4 and the default"""
    cp = curve(name)
    bases, lists, exp_lists, lengths, exp_lengths = indexed_batch(name, group)
    flat = [i for ix in lists for i in ix]
    for S in (1, 4, 0):
        got, _ = replay(hsb, cp, group, bases, [len(ix) for ix in lists], S, mode=1, index=flat)
        assert got == list(exp_lists), (name, group, S)
        got, _ = replay(hsb, cp, group, bases, lengths, S, mode=2)
        assert got == list(exp_lengths), (name, group, S)


def layout_check(hsb, lengths, S):
    stats = (ctypes.c_uint64 * 4)()
    rc = hsb.hsb_layout_check(c_offsets(lengths), len(lengths), S, stats)
    assert rc == 0, (rc, lengths, S)
    return tuple(stats)


def test_slices_read_every_index_exactly_once_and_chains_are_bounded(hsb):
    """the slice tables checked directly (hsb_layout_check): the case list and lengths around S, 32 S and 32^2 S, for every
    S the switch accepts up to 64 and for 4096"""
    for S in (1, 2, 4, 8, 16, 32, 64, 4096):
        shapes = [LENGTHS, [0], [0, 0, 0], [1], [S - 1 or 1, S, S + 1], [32 * S - 1, 32 * S, 32 * S + 1], [7] * 100 + [0] + [1] * 40]
        if S <= 8:
            shapes.append([32 * 32 * S + 1, 3, 32 * 32 * S])
        for lengths in shapes:
            slices, longest, group, passes = layout_check(hsb, lengths, S)
            assert slices == sum(-(-m // S) for m in lengths)
            assert longest <= S and group <= 32 and max(longest, group) <= max(S, 32)
            if sum(lengths):
                assert longest == min(S, max(lengths))
            most = max(-(-m // S) for m in lengths)
            want = 1
            while most > 32:
                most = -(-most // 32)
                want += 1
            assert passes == want, (lengths, S)


def test_default_slice_length_is_a_power_of_two_within_its_bounds(hsb):
    for group in (1, 2):
        lanes = min(MAX_LANES[group], 1 << 13)  # SUM_BATCH_FILL_SLICES: the slices from which on a longer slice wins
        seen = set()
        for total in [0, 1, 100, TOTAL] + [1 << e for e in range(10, 27)] + [(1 << e) - 1 for e in range(14, 24)]:
            for k in (1, 7, 1 << 10, 1 << 16):
                S = hsb.hsb_slice_default(total, k, group)
                seen.add(S)
                assert S in (4, 8, 16, 32), (total, k, group, S)
                assert hsb.hsb_slice_valid(S) == 1
                if S > 4:
                    assert total // S >= lanes  # the device is still full
                if S < 32:
                    assert total // (2 * S) < lanes  # ... and would not be at the next S
        assert seen == {4, 8, 16, 32}
    for v, ok in ((1, 1), (2, 1), (4096, 1), (0, 0), (3, 0), (-4, 0), (8192, 0), (48, 0)):
        assert hsb.hsb_slice_valid(v) == ok, v


def test_flagged_calls_check_their_arguments_before_they_ask_for_a_device(mlhip):
    lib = mlhip.load()
    pt, scb, out = bytes(192), bytes(32), ctypes.create_string_buffer(192)
    one = (ctypes.c_uint64 * 2)(0, 1)
    assert mlhip.SCALARS_UNIT == UNIT
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert re.search(r"^#define MLHIP_SCALARS_UNIT 0x400\b", hdr, re.M)

    def einval(rc, text):
        assert rc == mlhip.EINVAL and text in lib.mlhip_last_error(), (rc, lib.mlhip_last_error())

    def both(cid, group, p, offsets, k, o, text):
        einval(mlhip.mlhip_sum_batch(lib, cid, group, p, offsets, k, o), text)
        einval(mlhip.mlhip_sum_batch_device(lib, cid, group, p, offsets, k, o, None), text)

    # the flag beside a scalar array, and beside other bits of scalars_mont
    einval(lib.mlhip_msm_batch(1, 1, pt, scb, UNIT, one, 1, out), b"unit scalars take no scalar array")
    einval(lib.mlhip_msm_batch_device(1, 1, pt, scb, UNIT, one, 1, out, None), b"unit scalars take no scalar array")
    for mont in (UNIT | 1, UNIT | 2, UNIT | 0x100, UNIT | 0x800):
        einval(lib.mlhip_msm_batch(1, 1, pt, None, mont, one, 1, out), b"MLHIP_SCALARS_UNIT takes no other bit")
        einval(lib.mlhip_msm_batch_device(1, 1, pt, None, mont, one, 1, out, None), b"MLHIP_SCALARS_UNIT takes no other bit")
    # the handle forms check the handle first, as the plain calls
    einval(lib.mlhip_bases_msm_batch(None, None, UNIT, None, one, 1, out), b"null handle")
    einval(lib.mlhip_bases_msm_batch_device(None, None, UNIT, None, one, 1, None, out), b"null handle")
    # everything else is the plain call's rule and text
    for cid in (3, 7, -1):
        both(cid, 1, pt, one, 1, out, b"unknown curve id")
    for group in (0, 3, 0x101, -1):
        both(1, group, pt, one, 1, out, b"group must be 1 or 2")
    both(1, 1, pt, (ctypes.c_uint64 * 2)(1, 2), 1, out, b"msm batch: offsets[0] must be 0")
    both(1, 1, pt, (ctypes.c_uint64 * 3)(0, 2, 1), 2, out, b"msm batch: offsets decrease")
    both(1, 1, pt, None, 1, out, b"msm batch: offsets is null")
    both(1, 2, None, one, 1, out, b"null pointer")
    both(1, 2, pt, one, 1, None, b"null pointer")
    # K = 0 does nothing
    for cid in (0, 1, 2):
        for group in (1, 2):
            assert mlhip.mlhip_sum_batch(lib, cid, group, None, (ctypes.c_uint64 * 1)(0), 0, None) == 0
            assert mlhip.mlhip_sum_batch_device(lib, cid, group, None, (ctypes.c_uint64 * 1)(0), 0, None, None) == 0
    assert mlhip.sum_batch(1, 1, b"", []) == []
    assert out.raw == bytes(192)
    # a well-formed flagged call has no scalar array: without the feature this is MLHIP_EINVAL "null pointer"
    if mlhip.device_count() == 0:  # there is no CPU fallback
        assert mlhip.mlhip_sum_batch(lib, 1, 1, pt, one, 1, out) == mlhip.ENODEVICE
        # (host memory stands in for device memory: without a device the call returns before it reads any of it)
        assert mlhip.mlhip_sum_batch_device(lib, 1, 1, pt, one, 1, out, None) == mlhip.ENODEVICE
        assert mlhip.mlhip_sum_batch(lib, mlhip.CURVE_SUBGROUP_POINTS(1), 2, pt, one, 1, out) == mlhip.ENODEVICE
    else:
        assert mlhip.mlhip_sum_batch(lib, 1, 1, pt, one, 1, out) == 0  # one segment of one point at infinity
    assert out.raw == bytes(192)


def test_drivers_have_the_methods_and_the_abi_has_not_grown(mlhip):
    from mathlib_amd import build
    from mathlib_amd.driver import Bases, Curve

    assert callable(getattr(Curve, "SumG1Batch")) and callable(getattr(Curve, "SumG2Batch")) and callable(getattr(Bases, "SumBatch"))
    hpp = open(os.path.join(ROOT, "include", "mlhip_driver.hpp")).read()
    go = open(os.path.join(ROOT, "go", "driver", "hip", "hip.go")).read()
    for g in "12":
        assert re.search(r"std::vector<G%s> SumG%sBatch\(const std::vector<std::vector<G%s>>& lists\) const" % (g, g, g), hpp)
        assert re.search(r"^func \(c \*Curve\) SumG%sBatch\(a \[\]\[\]driver\.G%s\) \[\]driver\.G%s" % (g, g, g), go, re.M)
    assert re.search(r"std::vector<G1> SumBatch\(const std::vector<std::vector<uint32_t>>& index\) const", hpp)
    assert re.search(r"^func \(b \*Bases\) SumBatch\(index \[\]\[\]uint32, lengths \[\]int\) \[\]driver\.G1", go, re.M)
    assert "C.mlhip_sum_batch(" in go and "C.mlhip_bases_sum_batch(" in go and '#include "mlhip_sum_batch.h"' in go
    assert "mlhip_sum_batch(" in hpp and "mlhip_bases_sum_batch(" in hpp
    wrap = open(os.path.join(ROOT, "include", "mlhip_sum_batch.h")).read()
    for fn in ("mlhip_sum_batch", "mlhip_sum_batch_device", "mlhip_bases_sum_batch", "mlhip_bases_sum_batch_device"):
        assert re.search(r"^static inline int %s\(" % fn, wrap, re.M), fn
    assert "SumG1Batch" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fns = build.abi_functions()
    assert sorted(fns) == sorted(mlhip.SYMBOLS) and len(fns) == 77
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    table = hdr[hdr.index("---- environment switches") :]
    assert "MLHIP_SUM_BATCH_SLICE=s" in table
    # the flag is taken apart in the four batch entry points and nowhere else
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".h", ".hip", ".inc")) and "take_unit_scalars(" in open(os.path.join(csrc, f)).read())
    assert users == ["api_bases.hip", "api_msm.hip", "mlhip_rt.h"]
    calls = sum(open(os.path.join(csrc, f)).read().count("= take_unit_scalars(") for f in ("api_bases.hip", "api_msm.hip"))
    assert calls == 4
