"""The device route of mlhip_g1_sum / mlhip_g2_sum on the GPU (mathlib_amd/csrc/point_sum.h): the small lists of
tests/point_sum_cases.py pushed through the kernels (MLHIP_SUM_DEVICE_MIN=1) against oracle.pyref; random lists of 4 096,
4 097 and 2^16 + 1 points, device route against host route against cref.msm with unit scalars; 2^12 copies of one point
against [4096] P; the default threshold +- 1 with no switch set; and the Python and C++ drivers' SumG1 / SumG2."""
import ctypes
import functools
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_golden
from msm_batch_cases import neg_point
from oracle import cref
from point_sum_cases import COMPOSITIONS, CURVES, SIZES, case_bytes, curve, point_bytes

pytestmark = pytest.mark.gpu

ONE = (1).to_bytes(32, "little")
BIG = (1 << 16) + 1


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible"
    return l


def group_sum(lib, mlhip, cp, group, raw, n):
    out = ctypes.create_string_buffer(point_bytes(cp, group))
    fn = lib.mlhip_g1_sum if group == 1 else lib.mlhip_g2_sum
    mlhip.check(fn(cp.curve_id, raw, n, out))
    return out.raw


@functools.lru_cache(maxsize=None)
def random_list(name: str, group: int) -> bytes:
    """2^16 + 1 distinct points with points at infinity at the first, a middle and the last position of every prefix the
    tests take, and one point next to its negative"""
    cp = curve(name)
    ps = point_bytes(cp, group)
    raw = bytearray(cref.gen_points(cp.curve_id, group, 0x5EED + group, 0x1234567 + cp.curve_id, BIG))
    for i in (0, 2048, 4095, 4096, 40000, BIG - 1):
        raw[i * ps : (i + 1) * ps] = bytes(ps)
    raw[1001 * ps : 1002 * ps] = neg_point(cp, group, bytes(raw[1000 * ps : 1001 * ps]))
    raw[3000 * ps : 3001 * ps] = raw[2999 * ps : 3000 * ps]  # the same point twice
    return bytes(raw)


def default_threshold(group: int) -> int:
    src = open(os.path.join(ROOT, "mathlib_amd", "csrc", "api_msm.hip")).read()
    m = re.search(r"SUM_DEVICE_MIN_G%d = \(size_t\)1 << (\d+)" % group, src)
    assert m, "the default threshold of group %d" % group
    return 1 << int(m.group(1))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_small_lists_through_the_kernels(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "1")
    bad = []
    for kind in COMPOSITIONS:
        for n in SIZES:
            case = case_bytes(name, group, kind, n)
            if case is None:
                assert (name, group, kind) == ("BN254", 1, "outside_subgroup")
                continue
            raw, exp = case
            if group_sum(lib, mlhip, cp, group, raw, n) != exp:
                bad.append((kind, n))
    assert not bad, (name, group, bad)


@pytest.mark.parametrize("n", [4096, 4097, BIG])
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_device_route_equals_host_route_and_cref(lib, mlhip, monkeypatch, name, group, n):
    cp = curve(name)
    raw = random_list(name, group)[: n * point_bytes(cp, group)]
    monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "1")
    dev = group_sum(lib, mlhip, cp, group, raw, n)
    monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "0")
    host = group_sum(lib, mlhip, cp, group, raw, n)
    exp = cref.msm(cp.curve_id, group, raw, ONE * n, n, False, 0, 1)
    assert dev == host, (name, group, n)
    assert dev == exp, (name, group, n)
    assert any(dev)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_single_repeated_point(lib, mlhip, monkeypatch, name, group):
    """2^12 copies of P: every lane's second addition is the doubling branch, and the sum passes add equal partials"""
    cp = curve(name)
    ps = point_bytes(cp, group)
    p = cref.gen_points(cp.curve_id, group, 0xD0B1, 7, 1)[:ps]
    monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "1")
    got = group_sum(lib, mlhip, cp, group, p * 4096, 4096)
    assert got == cref.point_mul(cp.curve_id, group, p, 4096)
    # ... and P, -P alternating: every lane returns to infinity again and again
    pair = p + neg_point(cp, group, p)
    assert group_sum(lib, mlhip, cp, group, pair * 2048, 4096) == bytes(ps)
    assert group_sum(lib, mlhip, cp, group, pair * 2048 + p, 4097) == p


@pytest.mark.parametrize("group", [1, 2])
def test_default_threshold(lib, mlhip, monkeypatch, group):
    """no switch set: one below the default threshold (host loop), at it and one above (device route) give the host
    route's bytes"""
    name = "BLS12-381"
    cp = curve(name)
    t = default_threshold(group)
    assert 64 <= t < BIG and t & (t - 1) == 0
    for n in (t - 1, t, t + 1):
        raw = random_list(name, group)[: n * point_bytes(cp, group)]
        monkeypatch.delenv("MLHIP_SUM_DEVICE_MIN", raising=False)
        got = group_sum(lib, mlhip, cp, group, raw, n)
        monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "0")
        assert got == group_sum(lib, mlhip, cp, group, raw, n), (group, n)
    assert got == cref.msm(cp.curve_id, group, raw, ONE * n, n, False, 0, 1)


def test_argument_checks_keep_their_order(lib, mlhip, monkeypatch):
    monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "1")
    out = ctypes.create_string_buffer(192)
    for fn in (lib.mlhip_g1_sum, lib.mlhip_g2_sum):
        assert fn(9, None, 1, out) == mlhip.EINVAL and b"null" in lib.mlhip_last_error()
        assert fn(9, out, 1, None) == mlhip.EINVAL and b"null" in lib.mlhip_last_error()
        assert fn(9, out, 1, out) == mlhip.EINVAL and b"curve" in lib.mlhip_last_error()
        assert fn(1, None, 0, out) == 0 and out.raw == bytes(192)


def test_python_driver(lib, mlhip, monkeypatch):
    from mathlib_amd.driver import G1, G2, Curve

    for name in CURVES:
        cp = curve(name)
        cv = Curve(cp.curve_id)
        for group, el, fn in ((1, G1, cv.SumG1), (2, G2, cv.SumG2)):
            ps = point_bytes(cp, group)
            raw, exp = case_bytes(name, group, "infinities", 33)
            pts = [el(raw[i * ps : (i + 1) * ps], cv) for i in range(33)]
            monkeypatch.setenv("MLHIP_SUM_DEVICE_MIN", "1")
            assert fn(pts).raw == exp
            assert fn([]).IsInfinity()
            monkeypatch.delenv("MLHIP_SUM_DEVICE_MIN")
            assert fn(pts).raw == exp
            loop = pts[0].Copy()
            for p in pts[1:]:
                loop.Add(p)
            assert loop.raw == exp


def test_cpp_driver():
    src = os.path.join(ROOT, "tests", "cpp", "point_sum_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    so = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    exe = os.path.join(ROOT, "tests", "cpp", "point_sum_test")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(so)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    co = load_golden("BLS12-377")["g2_gen_coords"]
    env = {k: v for k, v in os.environ.items() if k != "MLHIP_SUM_DEVICE_MIN"}
    out = subprocess.run([exe, co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in CURVES:
        assert "%s sum_g1 6/6" % name in out.stdout
        assert "%s sum_g2 6/6" % name in out.stdout
