"""Prepared G2 handles without a GPU.  The device math of mathlib_amd/csrc/pairing_prepared.h, compiled for the CPU
(tests/hostmath_prepared): build the lines of fixed G2 points -> prepared Miller core -> the existing final_exp, over the
boundary-form element (the one-lane kernel's shape) and through the host models of the carry-free lane pair and quad (which
abort on any weight or value-bound violation), must equal oracle/pyref.py and the host-compiled miller_loop_core after the
final exponentiation -- every curve, 1 .. 4 pairs per product, infinities on either side, a Q outside G2, the pairing goldens.
Plus the argument errors of the C entry points that need no handle."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, load_golden
from g2_prepared_cases import CURVES, expand, g1_batch, g2_bytes, handle_points, index_forms
from oracle import pyref as R

NEW = ("mlhip_g2_prepared_create", "mlhip_g2_prepared_create_device", "mlhip_g2_prepared_count", "mlhip_g2_prepared_destroy",
       "mlhip_miller_loop_prepared", "mlhip_miller_loop_prepared_device", "mlhip_pairing_prepared", "mlhip_pairing_prepared_device")
FORMS = {"one-lane": 0, "lane-pair": 1, "quad": 2}


@pytest.fixture(scope="module")
def hp():
    import subprocess

    d = os.path.join(ROOT, "tests", "hostmath_prepared")
    so = os.path.join(d, "libhostmath_prepared.so")
    src = os.path.join(d, "prepared.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hp_prepared.argtypes = [ci, ci, vp, vp, ci, vp, ci, ci, vp]
    lib.hp_general.argtypes = [ci, vp, vp, ci, ci, vp]
    return lib


def prepared(hp, cp, form, g1, qs_bytes, m, index, ppp, fexp):
    out = ctypes.create_string_buffer(12 * cp.fp_bytes)
    idx = None if index is None else (ctypes.c_uint32 * ppp)(*index)
    rc = hp.hp_prepared(cp.curve_id, form, g1, qs_bytes, m, idx, ppp, 1 if fexp else 0, out)
    assert rc == 1, rc  # the largest weight left in the result
    return out.raw


def general(hp, cp, g1, g2, ppp, fexp):
    out = ctypes.create_string_buffer(12 * cp.fp_bytes)
    assert hp.hp_general(cp.curve_id, g1, g2, ppp, 1 if fexp else 0, out) == 1
    return out.raw


def oracle_fexp(cp, ps, qs):
    pairs = [(p, q) for p, q in zip(ps, qs) if p is not None and q is not None]
    return R.gt_to_mont_bytes(cp, R.final_exp(cp, R.miller_loop(cp, pairs)) if pairs else R.tower(cp).f12_one)


def test_line_count_matches_the_loop(hp):
    """doubling lines + one addition line per set bit below the top (+ BN254's two Frobenius lines)"""
    for name in CURVES:
        cp = R.CURVES[name]
        t = abs(6 * cp.x + 2) if name == "BN254" else abs(cp.x)
        want = (t.bit_length() - 1) + (bin(t).count("1") - 1) + (2 if name == "BN254" else 0)
        assert hp.hp_num_lines(cp.curve_id) == want, name
    assert hp.hp_num_lines(R.CURVES["BLS12-381"].curve_id) == 68


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", CURVES)
def test_prepared_pairing_matches_oracle_and_general_core(hp, name, form):
    """handle of 5 points (one at infinity, one outside G2), ppp = 1 .. 4, every q_index form, G1 infinities: after FExp the
    prepared loop gives the oracle's bytes and the host-compiled miller_loop_core's; fused (FExp inside) the same"""
    cp = R.CURVES[name]
    m = 5
    qs = handle_points(cp, m, "host")
    qb = g2_bytes(cp, qs)
    f = FORMS[form]
    for ppp in (1, 2, 3, 4):
        for fi, index in enumerate(index_forms(m, ppp)):
            ps, g1 = g1_batch(cp, 1, ppp, "host/%s/%d/%d" % (name, ppp, fi), inf_every=5 if fi == 1 else 0)
            eq = expand(qs, index, ppp, 1)
            want = oracle_fexp(cp, ps, eq)
            assert general(hp, cp, g1, g2_bytes(cp, eq), ppp, True) == want, (name, ppp, index)
            assert prepared(hp, cp, f, g1, qb, m, index, ppp, True) == want, (name, form, ppp, index)
            if form == "one-lane" or fi == 0:
                raw = prepared(hp, cp, f, g1, qb, m, index, ppp, False)
                assert R.gt_to_mont_bytes(cp, R.final_exp(cp, R.gt_from_mont_bytes(cp, raw))) == want, (name, form, ppp, index)


@pytest.mark.parametrize("name", CURVES)
def test_unscaled_lines_give_the_general_loops_raw_bytes(hp, name):
    """the lines are the general loop's own, unscaled: the raw Miller values agree too (not part of the contract)"""
    cp = R.CURVES[name]
    qs = handle_points(cp, 1, "raw")
    ps, g1 = g1_batch(cp, 1, 1, "raw/" + name, inf_every=0)
    want = general(hp, cp, g1, g2_bytes(cp, qs), 1, False)
    for f in FORMS.values():
        assert prepared(hp, cp, f, g1, g2_bytes(cp, qs), 1, None, 1, False) == want


@pytest.mark.parametrize("name", CURVES)
def test_infinities_on_either_side_give_one(hp, name):
    cp = R.CURVES[name]
    one = R.gt_to_mont_bytes(cp, R.tower(cp).f12_one)
    qs = handle_points(cp, 2, "inf")  # [Q, infinity]
    ps, g1 = g1_batch(cp, 1, 2, "inf/" + name, inf_every=0)
    g1n = 2 * cp.fp_bytes
    for f in FORMS.values():
        # the live pair alone decides; with both pairs dead the product is 1, raw and after FExp
        assert prepared(hp, cp, f, g1, g2_bytes(cp, qs), 2, None, 2, True) == oracle_fexp(cp, ps[:1], qs[:1])
        assert prepared(hp, cp, f, bytes(g1n) + g1[g1n:], g2_bytes(cp, qs), 2, None, 2, True) == one
        assert prepared(hp, cp, f, bytes(g1n) + g1[g1n:], g2_bytes(cp, qs), 2, None, 2, False) == one
        assert prepared(hp, cp, f, g1[:g1n], g2_bytes(cp, qs), 2, [1], 1, True) == one


@pytest.mark.parametrize("name", CURVES)
def test_pairing_goldens_through_a_one_point_handle(hp, name):
    cp = R.CURVES[name]
    for case in load_golden(name)["pairing"]:
        for f in FORMS.values():
            got = prepared(hp, cp, f, bytes.fromhex(case["g1"]), bytes.fromhex(case["g2"]), 1, None, 1, True)
            assert got.hex() == case["fexp"]


def test_header_declares_the_prepared_entry_points(mlhip):
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    for name in NEW:
        assert re.search(r"^MLHIP_API int %s\(" % name, hdr, re.M), name
    from mathlib_amd import build

    assert set(NEW) <= set(build.abi_functions())
    assert set(NEW) <= set(mlhip.SYMBOLS)


def test_argument_errors_that_need_no_handle(mlhip):
    """unknown curve, m = 0, null out-pointer, null handle: MLHIP_EINVAL with a message, before any device is touched; on a
    box without a GPU a valid create is MLHIP_ENODEVICE (there is no CPU fallback)"""
    lib = mlhip.load()
    cp = R.CURVES["BLS12-381"]
    q = g2_bytes(cp, handle_points(cp, 1, "args"))
    h = ctypes.c_void_p()

    def einval(rc):
        assert rc == mlhip.EINVAL and lib.mlhip_last_error()

    for create in (lib.mlhip_g2_prepared_create, lib.mlhip_g2_prepared_create_device):
        einval(create(7, q, 1, ctypes.byref(h)))
        einval(create(cp.curve_id, q, 0, ctypes.byref(h)))
        einval(create(cp.curve_id, q, 1, None))
        einval(create(cp.curve_id, None, 1, ctypes.byref(h)))
        assert not h.value
    m = ctypes.c_size_t()
    einval(lib.mlhip_g2_prepared_count(None, ctypes.byref(m)))
    out = ctypes.create_string_buffer(576)
    g1 = bytes(96)
    einval(lib.mlhip_miller_loop_prepared(None, g1, None, 1, 1, out))
    einval(lib.mlhip_pairing_prepared(None, g1, None, 1, 1, out))
    einval(lib.mlhip_miller_loop_prepared_device(None, None, None, 1, 1, None, None))
    einval(lib.mlhip_pairing_prepared_device(None, None, None, 1, 1, None, None))
    assert lib.mlhip_g2_prepared_destroy(None) == 0
    if mlhip.device_count() == 0:
        assert lib.mlhip_g2_prepared_create(cp.curve_id, q, 1, ctypes.byref(h)) == mlhip.ENODEVICE
        assert not h.value
