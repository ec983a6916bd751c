"""The device route of mlhip_g1_sum / mlhip_g2_sum without a GPU: the plan and the per-lane body of
mathlib_amd/csrc/point_sum.h, compiled for the CPU (tests/hostmath_sum), give oracle.pyref's sum for the lists of
tests/point_sum_cases.py on every curve and group; the plan's lanes read every index exactly once; the three drivers have
SumG1 / SumG2 and the C ABI has not grown; and without a device a long list is still summed (the host loop)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from point_sum_cases import COMPOSITIONS, CURVES, SIZES, case_bytes, curve, distinct_points, expected, ops, pack, point_bytes

MAX_LANES = {1: 65536, 2: 32768}


@pytest.fixture(scope="module")
def hms():
    d = os.path.join(ROOT, "tests", "hostmath_sum")
    so = os.path.join(d, "libpoint_sum_host.so")
    src = os.path.join(d, "point_sum_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hms_point_sum.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_uint32, vp, vp]
    lib.hms_plan_check.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32, vp]
    return lib


def replay(hms, cp, group, raw, n, force_l=0):
    out = ctypes.create_string_buffer(point_bytes(cp, group))
    stats = (ctypes.c_uint64 * 3)()
    rc = hms.hms_point_sum(cp.curve_id, group, raw, n, force_l, out, stats)
    assert rc == 0, rc
    return out.raw, tuple(stats)


def plan_check(hms, group, n, force_l=0):
    plan = (ctypes.c_uint64 * 3)()
    rc = hms.hms_plan_check(group, n, force_l, plan)
    assert rc == 0, (rc, group, n, force_l, tuple(plan))
    return tuple(plan)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_replayed_sums_match_pyref(hms, name, group):
    """every composition at every size, with the plan's L and with L forced to 1, 2 and 5 (long slices: the accumulator of
    one lane meets the repeated point, its negative and the infinities again and again)"""
    cp = curve(name)
    ps = point_bytes(cp, group)
    for kind in COMPOSITIONS:
        for n in SIZES:
            case = case_bytes(name, group, kind, n)
            if case is None:
                assert (name, group, kind) == ("BN254", 1, "outside_subgroup")
                continue
            raw, exp = case
            for force_l in (0, 1, 2, 5):
                got, (L, S, passes) = replay(hms, cp, group, raw, n, force_l)
                assert got == exp, (name, group, kind, n, force_l)
                assert S == -(-n // L) and passes >= 1
            if kind in ("all_infinity", "sums_to_infinity") or (kind == "pairs" and n % 2 == 0):
                assert exp == bytes(ps), (kind, n)  # the cases test what they claim
            elif kind in ("repeated", "outside_subgroup"):
                assert exp != bytes(ps), (kind, n)


def test_outside_subgroup_points_are_on_the_curve_and_outside():
    from oracle import pyref as R
    from point_sum_cases import outside_subgroup_point

    for name in CURVES:
        cp = curve(name)
        for group in (1, 2):
            x = outside_subgroup_point(name, group)
            if x is None:
                assert (name, group) == ("BN254", 1)
                continue
            if group == 1:
                assert R.g1_is_on_curve(cp, x) and R.g1_mul_unreduced(cp, x, cp.r) is not None
            else:
                assert R.g2_is_on_curve(cp, x) and R.g2_mul_unreduced(cp, x, cp.r) is not None


@pytest.mark.parametrize("group", [1, 2])
def test_plan_reads_every_index_exactly_once(hms, group):
    """n = 1, L - 1, L, L + 1, L S - 1, L S, L S + 1 around the plans of several sizes: with each n's own plan, and with L
    held at the base plan's (S is then the slice length of that L)"""
    seen_l = set()
    for base in (1, 31, 33, 1000, 4096, 5000, (1 << 16) + 1, 1 << 20, (1 << 22) + 3):
        L, S, chain = plan_check(hms, group, base)
        seen_l.add(L)
        assert 32 <= L <= MAX_LANES[group] and L & (L - 1) == 0
        assert S == -(-base // L)
        for n in (1, L - 1, L, L + 1, L * S - 1, L * S, L * S + 1):
            if n < 1:
                continue
            l2, s2, _ = plan_check(hms, group, n)
            assert s2 == -(-n // l2)
            lf, sf, _ = plan_check(hms, group, n, force_l=L)
            assert lf == L and sf == -(-n // L)
    assert len(seen_l) >= 4 and max(seen_l) == MAX_LANES[group]  # small lists take few lanes, large ones the whole machine


def test_plan_minimises_the_dependent_chain(hms):
    """no other power-of-two L between 32 and the machine's lanes gives a shorter chain of dependent additions"""
    for group in (1, 2):
        for n in (1, 100, 4096, 5000, 1 << 16, 1 << 20, 1 << 22):
            L, S, chain = plan_check(hms, group, n)
            l = 32
            while l <= MAX_LANES[group]:
                _, _, other = plan_check(hms, group, n, force_l=l)
                assert chain <= other, (group, n, L, l)
                if other == chain:
                    assert L <= l  # ties go to fewer lanes
                l *= 2


def test_drivers_have_the_methods_and_the_abi_has_not_grown(mlhip):
    from mathlib_amd import build
    from mathlib_amd.driver import Curve

    assert callable(getattr(Curve, "SumG1")) and callable(getattr(Curve, "SumG2"))
    hpp = open(os.path.join(ROOT, "include", "mlhip_driver.hpp")).read()
    go = open(os.path.join(ROOT, "go", "driver", "hip", "hip.go")).read()
    for name, fn in (("SumG1", "mlhip_g1_sum"), ("SumG2", "mlhip_g2_sum")):
        assert re.search(r"\bG[12] %s\(const std::vector<G[12]>& points\) const" % name, hpp), name
        assert re.search(r"^func \(c \*Curve\) %s\(a \[\]driver\.G[12]\) driver\.G[12]" % name, go, re.M), name
        assert "C.%s(" % fn in go
    assert "SumG1" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fns = build.abi_functions()
    assert sorted(fns) == sorted(mlhip.SYMBOLS) and len(fns) == 77
    assert "mlhip_g1_sum" in fns and "mlhip_g2_sum" in fns
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert "MLHIP_SUM_DEVICE_MIN" in hdr


@pytest.mark.parametrize("group", [1, 2])
def test_long_list_is_summed_with_or_without_a_device(mlhip, monkeypatch, group):
    """5 000 points with the threshold at 1: without a GPU the call must not fail with MLHIP_ENODEVICE but run the host
    loop; with one it takes the device route.  Either way the bytes are pyref's."""
    name = "BLS12-381"
    cp = curve(name)
    base = list(distinct_points(name, group))
    pts = (base * 25)[:5000]
    pts[17] = None
    raw = pack(cp, group, pts)
    add, _, to_bytes, _ = ops(cp, group)
    block = None
    for p in base:
        block = add(block, p)
    exp = None
    for _ in range(25):  # 25 times the 200 distinct points, less the one replaced by infinity
        exp = add(exp, block)
    exp = add(exp, ops(cp, group)[1](base[17]))
    monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "1")
    lib = mlhip.load()
    out = ctypes.create_string_buffer(point_bytes(cp, group))
    fn = lib.mlhip_g1_sum if group == 1 else lib.mlhip_g2_sum
    mlhip.check(fn(cp.curve_id, raw, len(pts), out))
    assert out.raw == to_bytes(exp)
    from mathlib_amd.driver import G1, G2, Curve

    cv = Curve(cp.curve_id)
    el = G1 if group == 1 else G2
    some = [el(raw[i * len(out.raw) : (i + 1) * len(out.raw)], cv) for i in range(40)]
    got = (cv.SumG1 if group == 1 else cv.SumG2)(some)
    assert got.raw == expected(cp, group, pts[:40])
    assert (cv.SumG1 if group == 1 else cv.SumG2)([]).IsInfinity()
