"""The Gt membership test and Gt.Inverse without a GPU.  The device math of mathlib_amd/csrc/gt_codec.h compiled for the CPU
(tests/hostmath_gtcodec): the membership chain and the Fp12 inverse over the plain tower and through the host models of the
carry-free lane pair and quad (which abort on any weight or value-bound violation), on every value of tests/gt_codec_cases.py
-- members, and values outside Gt of every kind the criterion has to tell apart -- against oracle/pyref.py, every curve.  Plus
the identities the criterion rests on, and the argument errors of the eight C entry points."""
import ctypes
import math
import os
import re

import pytest

from conftest import ROOT
from gt_codec_cases import CURVES, inverse_bytes, values, wires
from oracle import pyref as R

NEW = (
    "mlhip_gt_from_bytes",
    "mlhip_gt_from_bytes_device",
    "mlhip_gt_to_bytes",
    "mlhip_gt_to_bytes_device",
    "mlhip_gt_is_member",
    "mlhip_gt_is_member_device",
    "mlhip_gt_inverse",
    "mlhip_gt_inverse_device",
)
FORMS = {"tower": 0, "lane-pair": 1, "quad": 2}


@pytest.fixture(scope="module")
def gc():
    import subprocess

    d = os.path.join(ROOT, "tests", "hostmath_gtcodec")
    so = os.path.join(d, "libhostmath_gtcodec.so")
    src = os.path.join(d, "gtcodec.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gc_is_member.argtypes = [ci, ci, vp]
    lib.gc_inverse.argtypes = [ci, ci, vp, vp]
    return lib


@pytest.mark.parametrize("name", CURVES)
def test_the_criterion_is_exact(name):
    """gcd(Phi_12(p), p - lambda) = r with lambda = x (BLS12) / 6 x^2 (BN254): a value of the cyclotomic subgroup on which the
    Frobenius map is exponentiation by lambda has an order that divides r, and r is prime"""
    cp = R.CURVES[name]
    p = cp.p
    lam = 6 * cp.x * cp.x if name == "BN254" else cp.x
    phi = p**4 - p * p + 1
    assert phi % cp.r == 0 and (p - lam) % cp.r == 0
    assert math.gcd(phi, p - lam) == cp.r
    if name == "BN254":
        assert p - lam == cp.r
    else:
        assert phi % (p - lam) == (lam**4 - lam * lam + 1) % (p - lam) == cp.r


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", CURVES)
def test_membership_statuses_equal_the_oracle(gc, name, form):
    """every value of the case file; the models abort the process on a weight or value-bound violation, so reaching the
    assertion is the proof that there was none"""
    cp = R.CURVES[name]
    got = {v.label: gc.gc_is_member(cp.curve_id, FORMS[form], R.gt_to_mont_bytes(cp, v.f)) for v in values(name)}
    assert got == {v.label: int(v.member) for v in values(name)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", CURVES)
def test_inverse_times_value_is_one_and_zero_maps_to_zero(gc, name, form):
    cp = R.CURVES[name]
    T = R.tower(cp)
    out = ctypes.create_string_buffer(12 * cp.fp_bytes)
    for v in values(name):
        assert gc.gc_inverse(cp.curve_id, FORMS[form], R.gt_to_mont_bytes(cp, v.f), out) == 0
        assert out.raw == inverse_bytes(name)[v.label], (name, form, v.label)
        inv = R.gt_from_mont_bytes(cp, out.raw)
        if v.label == "zero":
            assert out.raw == bytes(12 * cp.fp_bytes)
        else:
            assert T.f12_is_one(T.f12_mul(inv, v.f)), (name, form, v.label)
        if v.member:
            assert inv == T.f12_conj(v.f)


@pytest.mark.parametrize("name", CURVES)
def test_case_file_covers_what_the_gpu_tests_need(name):
    cp = R.CURVES[name]
    ws = wires(name)
    assert len(ws) == 16 and [w.status for w in ws].count(0) == 5 and [w.status for w in ws].count(1) == 4
    for w in ws:
        assert len(w.wire) == 12 * cp.fp_bytes
        coords = [int.from_bytes(w.wire[k * cp.fp_bytes : (k + 1) * cp.fp_bytes], "big") for k in range(12)]
        assert (max(coords) >= cp.p) == (w.status == 1)


def test_header_declares_the_entry_points(mlhip):
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    for name in NEW:
        assert re.search(r"^MLHIP_API int %s\(int curve_id," % name, hdr, re.M), name
    from mathlib_amd import build

    assert set(NEW) <= set(build.abi_functions()) and set(NEW) <= set(mlhip.SYMBOLS)
    assert len(build.abi_functions()) == 77


def test_argument_errors_come_before_the_device(mlhip):
    """unknown curve and null pointers: MLHIP_EINVAL with a message before any device is touched; n = 0 does nothing; on a box
    without a GPU a valid call is MLHIP_ENODEVICE (there is no CPU fallback)"""
    lib = mlhip.load()
    gt, out, st = bytes(576), ctypes.create_string_buffer(576), ctypes.create_string_buffer(1)
    # (arguments after the curve id, indices of the pointers among them)
    calls = {
        "mlhip_gt_from_bytes": ([gt, 1, 1, out, st], (0, 3, 4)),
        "mlhip_gt_from_bytes_device": ([gt, 1, 1, out, st, None], (0, 3, 4)),
        "mlhip_gt_to_bytes": ([gt, 1, out], (0, 2)),
        "mlhip_gt_to_bytes_device": ([gt, 1, out, None], (0, 2)),
        "mlhip_gt_is_member": ([gt, 1, st], (0, 2)),
        "mlhip_gt_is_member_device": ([gt, 1, st, None], (0, 2)),
        "mlhip_gt_inverse": ([gt, 1, out], (0, 2)),
        "mlhip_gt_inverse_device": ([gt, 1, out, None], (0, 2)),
    }
    assert set(calls) == set(NEW)

    def einval(rc):
        assert rc == mlhip.EINVAL and lib.mlhip_last_error()

    for name, (args, ptrs) in calls.items():
        fn = getattr(lib, name)
        einval(fn(9, *args))
        for k in ptrs:
            einval(fn(1, *[None if j == k else a for j, a in enumerate(args)]))
        zero = [0 if j == 1 else (None if j in ptrs else a) for j, a in enumerate(args)]
        assert fn(1, *zero) == 0, name
        if mlhip.device_count() == 0:
            # (host memory stands in for device memory: without a device the call returns before it reads any of it)
            assert fn(1, *args) == mlhip.ENODEVICE, name
    if mlhip.device_count() == 0:
        assert out.raw == bytes(576) and st.raw == bytes(1)
