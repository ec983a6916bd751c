"""mlhip_msm_batch / mlhip_msm_batch_device for points promised in G1 / G2 (MLHIP_CURVE_SUBGROUP_POINTS) without a GPU.  The
two chunk bodies of mathlib_amd/csrc/msm_batch_endo.h compiled for the CPU (tests/hostmath_batch_endo) give cref.msm's bytes
for every segment -- every (curve, group) that has a split, every compiled chunk length, chunks shorter than P, the scalars
on the digit boundaries of the split in both scalar forms, unreduced scalars, infinities, the degenerate pairs of
tests/msm_batch_cases.py and the ones the endomorphism adds -- and, for a point OUTSIDE the subgroup, a value that is not
the product (what makes the route visible on the GPU).  Plus the argument rules of the two entry points that take the
promise, which need no device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from msm_batch_cases import edge_segments, expected, point_bytes, random_segments
from msm_batch_subgroup_cases import (CHUNKS, CURVES, SPLIT, endo_edge_segments, endo_scalar, harness, host_batch, mul,
                                      scalar_segments, to_bytes)
from oracle import pyref as R
from point_sum_cases import distinct_points, outside_subgroup_point


@pytest.fixture(scope="module")
def hbe():
    return harness()


def test_which_groups_and_chunk_lengths_have_a_split_body(hbe):
    for name, cid in CURVES.items():
        cp = R.CURVES[name]
        for group in (1, 2):
            for P in (1, 2, 4, 8):
                rc, out = host_batch(hbe, cp, group, P, b"", b"", [0], False)
                if (name, group) not in SPLIT:
                    assert rc == -3
                elif P not in CHUNKS[group]:
                    assert rc == -5  # G2 at P = 8: the plain chunk kernel
                else:
                    assert rc == 0 and out == [bytes(point_bytes(cp, group))]


@pytest.mark.parametrize("name,group", SPLIT)
def test_segments_of_every_length_and_chunk(hbe, name, group):
    """lengths 0, 1, P - 1, P, P + 1, 17 and 64 over uniform 256-bit scalars (mostly unreduced), both scalar forms"""
    cp = R.CURVES[name]
    for P in CHUNKS[group]:
        lengths = [0, 1, max(P - 1, 0), P, P + 1, 3, 0, 17, 64]
        pts, scs, lengths = random_segments(cp, group, lengths, "subgroup-host/%s/%d/%d" % (name, group, P))
        for mont in (False, True):
            rc, got = host_batch(hbe, cp, group, P, pts, scs, lengths, mont)
            assert rc == 0 and got == expected(cp, group, pts, scs, lengths, mont), (name, group, P, mont)


@pytest.mark.parametrize("name,group", SPLIT)
def test_scalars_on_the_boundaries_of_the_split(hbe, name, group):
    cp = R.CURVES[name]
    for mont in (0, 1):
        pts, scs, lengths = scalar_segments(name, group, mont)
        exp = expected(cp, group, pts, scs, list(lengths), bool(mont))
        for P in CHUNKS[group]:
            rc, got = host_batch(hbe, cp, group, P, pts, scs, list(lengths), bool(mont))
            assert rc == 0 and got == exp, (name, group, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])


@pytest.mark.parametrize("name,group", SPLIT)
def test_degenerate_pairs_inside_one_chunk(hbe, name, group):
    cp = R.CURVES[name]
    ps = point_bytes(cp, group)
    for make in (edge_segments, endo_edge_segments):
        for pad in (0, 1, 3):
            pts, scs, lengths = make(cp, group, "subgroup-host-edge/%s/%d" % (name, group), pad)
            for mont in (False, True):
                exp = expected(cp, group, pts, scs, lengths, mont)
                for P in CHUNKS[group]:
                    rc, got = host_batch(hbe, cp, group, P, pts, scs, lengths, mont)
                    assert rc == 0 and got == exp, (make.__name__, name, group, pad, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])
    # the new cases test what they claim: the cancellations are the point at infinity, the meeting pairs are [2 d]Q
    pts, scs, lengths = endo_edge_segments(cp, group, "subgroup-host-edge/%s/%d" % (name, group), 0)
    exp = expected(cp, group, pts, scs, lengths, False)
    assert exp[2] == bytes(ps) and exp[7] == bytes(ps)
    d = int.from_bytes(scs[32:64], "little")
    Q = mul(cp, group, distinct_points(name, group, 300)[7], endo_scalar(cp, group) % cp.r)
    assert pts[ps : 2 * ps] == to_bytes(cp, group, Q)
    assert exp[0] == exp[1] == to_bytes(cp, group, mul(cp, group, Q, 2 * d))


@pytest.mark.parametrize("name,group", SPLIT)
def test_point_outside_the_subgroup_gives_the_endomorphism_not_the_product(hbe, name, group):
    """s = x^2 (G1: a = 0, b = 1) / |x| or 6 x^2 (G2: the digit d1 = 1) on a point T outside the subgroup, between two pairs of
    the subgroup: the chunk adds the endomorphism's image of T, which is not [s]T -- G1: exactly (beta x, -y)"""
    cp = R.CURVES[name]
    T = outside_subgroup_point(name, group)
    s = endo_scalar(cp, group)
    base = distinct_points(name, group, 300)
    pts = b"".join(to_bytes(cp, group, p) for p in (base[1], T, base[2]))
    scs = b"".join(v.to_bytes(32, "little") for v in (5, s, 7))
    add = R.g1_add if group == 1 else R.g2_add
    unreduced = R.g1_mul_unreduced if group == 1 else R.g2_mul_unreduced
    rest = add(cp, mul(cp, group, base[1], 5), mul(cp, group, base[2], 7))
    true = to_bytes(cp, group, add(cp, rest, unreduced(cp, T, s)))
    for P in CHUNKS[group]:
        rc, got = host_batch(hbe, cp, group, P, pts, scs, [3], False)
        assert rc == 0 and got[0] != true, (name, group, P)
        if group == 1:
            Q = R.g1_mul(cp, base[1], s)
            beta = Q[0] * pow(base[1][0], -1, cp.p) % cp.p
            assert got[0] == to_bytes(cp, group, add(cp, rest, (beta * T[0] % cp.p, cp.p - T[1])))
    # the other segments of a batch do not see it
    rc, got = host_batch(hbe, cp, group, 2, pts, scs, [1, 1, 1], False)
    assert rc == 0 and got[0] == to_bytes(cp, group, mul(cp, group, base[1], 5)) and got[2] == to_bytes(cp, group, mul(cp, group, base[2], 7))


# ---- the C ABI: no GPU needed ------------------------------------------------------------------------------------------


def test_headers_carry_the_macro_and_the_wrappers(mlhip):
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert re.search(r"^#define MLHIP_CURVE_SUBGROUP_POINTS\(curve_id\) \(\(curve_id\) >= 0 && \(curve_id\) <= 2 \? \(\(curve_id\) \| 0x100\) : -1\)$",
                     hdr, re.M)
    assert "MLHIP_MSM_BATCH_ENDO=0" in hdr
    wrap = open(os.path.join(ROOT, "include", "mlhip_subgroup.h")).read()
    for name in ("mlhip_msm_batch_subgroup", "mlhip_msm_batch_subgroup_device"):
        assert re.search(r"^static inline int %s\(int curve_id, int group," % name, wrap, re.M), name
    assert [mlhip.CURVE_SUBGROUP_POINTS(c) for c in (0, 1, 2)] == [0x100, 0x101, 0x102]
    assert mlhip.CURVE_SUBGROUP_POINTS(-1) == mlhip.CURVE_SUBGROUP_POINTS(3) == mlhip.CURVE_SUBGROUP_POINTS(0x101) == -1


def test_dynamic_symbol_table_is_unchanged(mlhip):
    """the promise travels in the curve id: 77 functions, the ones the header declares"""
    import subprocess

    from mathlib_amd import build

    out = subprocess.check_output(["nm", "-D", "--defined-only", mlhip.LIB_PATH], text=True)
    names = sorted(line.split()[-1].split("@")[0] for line in out.splitlines() if " T " in line)
    assert names == build.abi_functions() and len(names) == 77


def test_flagged_call_with_no_segments_returns_zero(mlhip):
    """K = 0 does nothing, as in the plain call (an unknown curve id, MLHIP_EINVAL, before the flag existed)"""
    lib = mlhip.load()
    offsets = (ctypes.c_uint64 * 1)(0)
    for cid in (0, 1, 2):
        for group in (1, 2):
            assert mlhip.msm_batch_subgroup(lib, cid, group, None, None, 0, offsets, 0, None) == 0
            assert mlhip.msm_batch_subgroup_device(lib, cid, group, None, None, 0, offsets, 0, None, None) == 0
    assert mlhip.msm_batch(1, 1, b"", b"", False, [], subgroup=True) == []


def test_flagged_calls_check_their_arguments_as_the_plain_calls(mlhip):
    lib = mlhip.load()
    pt, scb, out = bytes(192), bytes(32), ctypes.create_string_buffer(192)
    one = (ctypes.c_uint64 * 2)(0, 1)

    def einval(rc, text=None):
        assert rc == mlhip.EINVAL and lib.mlhip_last_error()
        if text:
            assert text in lib.mlhip_last_error()

    def both(cid, group, p, s, offsets, k, o, text=None):
        einval(mlhip.msm_batch_subgroup(lib, cid, group, p, s, 0, offsets, k, o), text)
        einval(mlhip.msm_batch_subgroup_device(lib, cid, group, p, s, 0, offsets, k, o, None), text)

    # the wrappers take a plain curve id: anything else, a flagged value included, makes the macro -1
    for cid in (3, 7, -1, 0x100, 0x101, 0x102):
        both(cid, 1, pt, scb, one, 1, out, b"unknown curve id")
    # a flag on any other curve id is no promise
    for cid in (0x103, 0x1FF, 0x200, 0x201, 0x1101):
        einval(lib.mlhip_msm_batch(cid, 1, pt, scb, 0, one, 1, out), b"unknown curve id")
        einval(lib.mlhip_msm_batch_device(cid, 1, pt, scb, 0, one, 1, out, None), b"unknown curve id")
    for group in (0, 3, 0x101, 0x102, -1):
        both(1, group, pt, scb, one, 1, out, b"group must be 1 or 2")
    for offsets, k in (((ctypes.c_uint64 * 2)(1, 2), 1), ((ctypes.c_uint64 * 3)(0, 2, 1), 2), (None, 1)):
        both(1, 1, pt, scb, offsets, k, out)
    for p, s, o in ((None, scb, out), (pt, None, out), (pt, scb, None)):
        both(1, 2, p, s, one, 1, o, b"null pointer")
    if mlhip.device_count() == 0:  # there is no CPU fallback
        assert mlhip.msm_batch_subgroup(lib, 1, 1, pt, scb, 0, one, 1, out) == mlhip.ENODEVICE
        # (host memory stands in for device memory: without a device the call returns before it reads any of it)
        assert mlhip.msm_batch_subgroup_device(lib, 1, 1, pt, scb, 0, one, 1, out, None) == mlhip.ENODEVICE
    assert out.raw == bytes(192)


def test_other_entry_points_still_take_the_flagged_curve_id_for_an_unknown_curve(mlhip):
    lib = mlhip.load()
    pt, scb, out = bytes(192), bytes(32), ctypes.create_string_buffer(192)
    plan, bases = ctypes.c_void_p(), ctypes.c_void_p()
    calls = {
        "scalar_mul": lambda c: lib.mlhip_scalar_mul(c, 1, pt, 1, scb, 0, 1, out),
        "msm_plan_create": lambda c: lib.mlhip_msm_plan_create(c, 1, 16, 0, ctypes.byref(plan)),
        "bases_create": lambda c: lib.mlhip_bases_create(c, 1, pt, 1, 0, ctypes.byref(bases)),
        "msm_g1": lambda c: lib.mlhip_msm_g1(c, pt, scb, 0, 1, 0, out),
    }
    for name, call in calls.items():
        assert call(7) == mlhip.EINVAL
        want = lib.mlhip_last_error()
        assert b"unknown curve id" in want, name
        for flagged in (0x100, 0x101, 0x102):
            assert call(flagged) == mlhip.EINVAL and lib.mlhip_last_error() == want, name
    assert not plan.value and not bases.value and out.raw == bytes(192)
