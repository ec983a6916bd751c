"""Gt.Exp for members of Gt without a GPU.  The device math of mathlib_amd/csrc/gt_exp_cyclo.h and pairing_quad.h's
fp12q_cyclo_sqr, compiled for the CPU (tests/hostmath_gtexp): the scalar split against Python integers, the quad Granger-Scott
squaring against the generic quad squaring, and the whole chain through the host models of the carry-free lane pair and quad
(which abort on any weight or value-bound violation) against oracle/pyref.py's f12_pow -- every curve.  The 4-bit windowed
chain of mlhip_gt_exp (gt_exp_window_chain) the same way, over the plain tower too and on a value outside Gt.  Plus the
argument errors of the two C entry points."""
import ctypes
import functools
import os
import re

import pytest

from conftest import ROOT
from gt_exp_cyclo_cases import CURVES, boundary_scalars, digits, member, member_pow, split_modulus
from oracle import pyref as R

NEW = ("mlhip_gt_exp_cyclo", "mlhip_gt_exp_cyclo_device")
FORMS = {"lane-pair": 1, "quad": 2}


@pytest.fixture(scope="module")
def gx():
    import subprocess

    d = os.path.join(ROOT, "tests", "hostmath_gtexp")
    so = os.path.join(d, "libhostmath_gtexp.so")
    src = os.path.join(d, "gtexp.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gx_modulus.argtypes = [ci, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.gx_split.argtypes = [ci, vp, ci, vp, vp]
    lib.gx_cyclo_sqr.argtypes = [ci, vp, vp, vp]
    lib.gx_exp.argtypes = [ci, ci, vp, vp, ci, vp]
    lib.gx_exp_window.argtypes = [ci, ci, vp, vp, ci, vp]
    return lib


def split(gx, cp, s, mont):
    """(digits, canonical scalar) as the kernels compute them; mont = -1: the split of s as it is"""
    dig = ctypes.create_string_buffer(32)
    canon = ctypes.create_string_buffer(32)
    raw = R.scalar_to_bytes(s, cp, mont=True) if mont == 1 else s.to_bytes(32, "little")
    dim = gx.gx_split(cp.curve_id, raw, mont, dig, canon)
    assert dim == split_modulus(cp)[1]
    nb = 32 // dim
    return [int.from_bytes(dig.raw[i * nb : (i + 1) * nb], "little") for i in range(dim)], int.from_bytes(canon.raw, "little")


@pytest.mark.parametrize("name", CURVES)
def test_frobenius_is_exponentiation_by_the_split_modulus(gx, name):
    """what the split rests on: p = x (BLS12) / 6 x^2 (BN254) mod r, the modulus the device code uses is that value's
    magnitude, and the digit bounds the issue states"""
    cp = R.CURVES[name]
    lam, dim = split_modulus(cp)
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    assert gx.gx_modulus(cp.curve_id, ctypes.byref(lo), ctypes.byref(hi)) == dim
    assert lo.value + (hi.value << 64) == lam
    if name == "BN254":
        assert cp.p % cp.r == lam and lam < 1 << 127 and lam * lam < cp.r
        assert (cp.r - 1) // lam > lam and (cp.r - 1) // lam < 1 << 127  # the top digit exceeds L and still fits
    else:
        assert (cp.p - cp.x) % cp.r == 0 and lam < 1 << 64 and cp.r < lam**4
        assert (cp.r - 1) // lam**3 < 1 << 64


@pytest.mark.parametrize("name", CURVES)
def test_digit_split_matches_python_integers(gx, name):
    cp = R.CURVES[name]
    lam, dim = split_modulus(cp)
    scalars = boundary_scalars(cp)
    assert lam**dim - 1 in scalars and cp.r - 1 in scalars
    for s in scalars:
        got, canon = split(gx, cp, s, -1)
        assert canon == s and got == digits(cp, s), (name, hex(s))
        assert sum(d * lam**i for i, d in enumerate(got)) == s
        for mont in (0, 1):  # behind fr_canonical, as the kernels run it: the digits of s mod r
            got, canon = split(gx, cp, s, mont)
            assert canon == s % cp.r and got == digits(cp, s % cp.r), (name, hex(s), mont)
    assert digits(cp, lam**dim - 1) == [lam - 1] * dim
    if name == "BN254":
        assert split(gx, cp, cp.r - 1, 0)[0][1] > lam
    d = R.Drbg("gt_exp_cyclo/split/" + name)
    for _ in range(20):
        s = d.below(1 << 256)
        got, canon = split(gx, cp, s, 0)
        assert canon == s % cp.r and got == digits(cp, canon)


@pytest.mark.parametrize("name", CURVES)
def test_quad_cyclotomic_squaring_equals_the_generic_one(gx, name):
    """on an FExp output and on 1; the host model aborts on a weight or value-bound violation (u^2 = -5 and the 10-limb
    curve included), and the results come out with weight 1"""
    cp = R.CURVES[name]
    T = R.tower(cp)
    for f in (member(name), T.f12_one):
        a = ctypes.create_string_buffer(12 * cp.fp_bytes)
        b = ctypes.create_string_buffer(12 * cp.fp_bytes)
        assert gx.gx_cyclo_sqr(cp.curve_id, R.gt_to_mont_bytes(cp, f), a, b) == 1
        assert a.raw == b.raw == R.gt_to_mont_bytes(cp, T.f12_sqr(f))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", CURVES)
def test_chain_matches_f12_pow(gx, name, form):
    """two Gt members per curve (a pairing of DRBG points, and 1), the boundary scalars of the split and unreduced ones"""
    cp = R.CURVES[name]
    T = R.tower(cp)
    one = R.gt_to_mont_bytes(cp, T.f12_one)
    base = R.gt_to_mont_bytes(cp, member(name))
    scalars = boundary_scalars(cp) + [cp.r, cp.r + 1, 2 * cp.r + 3, (1 << 256) - 1, 0x1234567 << 200 | 0xABCDEF]
    out = ctypes.create_string_buffer(12 * cp.fp_bytes)
    for k, s in enumerate(scalars):
        mont = k & 1
        raw = R.scalar_to_bytes(s, cp, mont=True) if mont else s.to_bytes(32, "little")
        assert gx.gx_exp(cp.curve_id, FORMS[form], base, raw, mont, out) == 1
        assert out.raw == member_pow(name, s % cp.r), (name, form, hex(s))
        if k < 6:
            assert gx.gx_exp(cp.curve_id, FORMS[form], one, raw, mont, out) == 1
            assert out.raw == one


@functools.lru_cache(maxsize=None)
def window_cases(name):
    """(base bytes, [(scalar, expected bytes)]) for a member of Gt and for an arbitrary Fp12 value: the scalars 0, 1, 15, 16
    (one window, and the first carry into the second), r - 1, two random ones, and one whose top nibble is zero while the
    next is not (the chain starts at the second window)"""
    cp = R.CURVES[name]
    T = R.tower(cp)
    d = R.Drbg("gt_exp_window/" + name)
    top_nibble_zero = (d.below(1 << 252) | 1 << 251) % (1 << 252)
    assert top_nibble_zero >> 252 == 0 and top_nibble_zero >> 248 != 0 and top_nibble_zero < cp.r
    scalars = [0, 1, 15, 16, cp.r - 1, d.below(cp.r), d.below(cp.r), top_nibble_zero]
    arbitrary = T.f12_mul(member(name), T.f12_add(member(name), T.f12_one))  # f (f + 1): a unit of Fp12 outside Gt
    assert T.f12_pow(arbitrary, cp.r) != T.f12_one
    return [(R.gt_to_mont_bytes(cp, f), [(s, R.gt_to_mont_bytes(cp, T.f12_pow(f, s))) for s in scalars]) for f in (member(name), arbitrary)]


@pytest.mark.parametrize("form", ["plain"] + list(FORMS))
@pytest.mark.parametrize("name", CURVES)
def test_window_chain_matches_f12_pow(gx, name, form):
    """the chain of mlhip_gt_exp's kernels on the host: right for a member of Gt and for any other Fp12 value, and the
    carry-free models stay within their budgets (they abort otherwise) and hand back weight 1"""
    cp = R.CURVES[name]
    out = ctypes.create_string_buffer(12 * cp.fp_bytes)
    for base, rows in window_cases(name):
        for k, (s, want) in enumerate(rows):
            mont = k & 1
            raw = R.scalar_to_bytes(s, cp, mont=True) if mont else s.to_bytes(32, "little")
            assert gx.gx_exp_window(cp.curve_id, FORMS.get(form, 0), base, raw, mont, out) == 1
            assert out.raw == want, (name, form, hex(s))


def test_header_declares_the_entry_points(mlhip):
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    for name in NEW:
        assert re.search(r"^MLHIP_API int %s\(int curve_id," % name, hdr, re.M), name
    from mathlib_amd import build

    assert set(NEW) <= set(build.abi_functions()) and set(NEW) <= set(mlhip.SYMBOLS)


def test_argument_errors_come_before_the_device(mlhip):
    """unknown curve and null pointers: MLHIP_EINVAL with a message before any device is touched; n = 0 does nothing; on a box
    without a GPU a valid call is MLHIP_ENODEVICE (there is no CPU fallback)"""
    lib = mlhip.load()
    gt, sc, out = bytes(576), bytes(32), ctypes.create_string_buffer(576)

    def einval(rc):
        assert rc == mlhip.EINVAL and lib.mlhip_last_error()

    einval(lib.mlhip_gt_exp_cyclo(7, gt, sc, 0, 1, out))
    einval(lib.mlhip_gt_exp_cyclo_device(7, gt, sc, 0, 1, out, None))
    for args in ((None, sc, out), (gt, None, out), (gt, sc, None)):
        einval(lib.mlhip_gt_exp_cyclo(1, args[0], args[1], 0, 1, args[2]))
        einval(lib.mlhip_gt_exp_cyclo_device(1, args[0], args[1], 0, 1, args[2], None))
    assert lib.mlhip_gt_exp_cyclo(1, None, None, 0, 0, None) == 0
    assert lib.mlhip_gt_exp_cyclo_device(1, None, None, 0, 0, None, None) == 0
    if mlhip.device_count() == 0:
        assert lib.mlhip_gt_exp_cyclo(1, gt, sc, 0, 1, out) == mlhip.ENODEVICE
        # (host memory stands in for device memory: without a device the call returns before it reads any of it)
        assert lib.mlhip_gt_exp_cyclo_device(1, gt, sc, 0, 1, out, None) == mlhip.ENODEVICE
    assert out.raw == bytes(576)
