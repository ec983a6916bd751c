"""The CPU half of the device field-arithmetic tests (tests/test_devmath_gpu.py): the harness still cross-compiles, the
operand generator only emits what the ops accept, the Python transcription of fp28.h agrees with the host-compiled
portable form, and the two generated .inc files are what their generators print.  Nothing here launches a kernel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import devmath_cases as D
from devmath_cases import ROOT, build_harness

CURVES = D.CURVES


def test_harness_cross_compiles_in_both_forms():
    """compile and link only: keeps tests/devmath/devmath.hip from rotting between GPU visits"""
    for portable in (False, True):
        so = build_harness(portable)
        syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        assert " T dm_run" in syms and " T dm_fp28_is_asm" in syms, so
        assert "mlhip_" not in syms  # a test artefact: none of the library's ABI


@pytest.mark.parametrize("name", CURVES)
def test_operands_respect_every_contract(name):
    """check_preconditions for every emitted vector of every op; the structured blocks do reach the region just under
    2^63 (above 2^62) that uniformly random points never see"""
    for op in D.ALL_OPS:
        worst = D.check_preconditions(name, op)
        assert worst < D.LIM63
        if op in ("fp28_mul", "fp28_mul2"):
            assert worst > 1 << 62, (name, op, worst)
    assert sorted(D.mul2_weights()) == sorted({(a, b, c, d) for a in range(1, 9) for b in range(1, 9) for c in range(1, 9) for d in range(1, 9)
                                               if a * b + c * d == 8})


def test_precondition_check_rejects_what_the_contract_excludes():
    """the check is a condition, not a measurement: operands one step outside are refused"""
    F = D.field("BLS12-381")
    e3 = D.limb_array([[4 * D.B28 - 1] * (F.L - 1) + [0]])
    assert int(D.column_magnitudes(F, "fp28_mul", (e3, e3))[0]) >= D.LIM63  # w_a w_b = 16
    with pytest.raises(OverflowError):
        D.mont_py(F, [int(x) for x in e3[0]], [int(x) for x in e3[0]])
    assert not D.has_weight(F, D.limb_array([[D.B28] + [0] * (F.L - 1)]), 1)[0]
    assert not D.is_normalized(F, D.limb_array([D.limbs_of(F.norm_hi, F.L)]))[0]
    assert not D.is_normalized(F, D.limb_array([D.limbs_of(F.norm_lo - 1, F.L)]))[0]
    assert D.is_normalized(F, D.limb_array([D.limbs_of(F.norm_hi - 1, F.L), D.limbs_of(F.norm_lo, F.L)])).all()


def _host_raw(hostmath, F, op, operands, idx):
    """hm_fp28_raw over the vectors idx: (out, out2) as int32 / uint32 arrays"""
    code = D.OPS[op]
    out_w = F.N if op == "fp28_to_fp" else F.L
    o1 = np.zeros((len(idx), out_w), dtype=np.int32)
    o2 = np.zeros((len(idx), out_w), dtype=np.int32)
    P = ctypes.c_void_p
    hostmath.hm_fp28_raw.argtypes = [ctypes.c_int, ctypes.c_int] + [P] * 6
    ops = [np.ascontiguousarray(a) for a in operands]
    for r, i in enumerate(idx):
        ptr = [a[i].ctypes.data for a in ops] + [None] * (4 - len(ops))
        assert hostmath.hm_fp28_raw(F.cid, code, *ptr, o1[r].ctypes.data, o2[r].ctypes.data) == 0
    return (o1.view(np.uint32), o2) if op == "fp28_to_fp" else (o1, o2)


@pytest.mark.parametrize("name", CURVES)
def test_transcription_and_predicates_against_host_portable_form(hostmath, name):
    """Python integers <-> host portable: on the whole structured block the host-compiled fp28_mont / fp28_k2mul_portable
    give the right residue and a normalized result; on the structured sample their limbs equal the Python transcription's.
    fp28_reduce, fp28_normalize and the boundary conversions likewise (all three curves)."""
    F = D.field(name)
    for op in ("fp28_mul", "fp28_sqr", "fp28_mul2", "fp28_k2mul"):
        cs = D.cases(name, op)
        idx = np.arange(cs.n_struct)
        outs = _host_raw(hostmath, F, op, cs.operands, idx)
        vals = [D.values(a[: cs.n_struct]) for a in cs.operands]
        for k, want in enumerate(D.product_integers(op, vals)):
            assert ((D.values(outs[k]) * F.R28 - want) % F.p == 0).all(), (name, op)
            assert D.is_normalized(F, outs[k]).all(), (name, op)
        for i in cs.sample:
            ref = D.transcription(F, op, [[int(x) for x in o[i]] for o in cs.operands])
            for k in range(len(ref)):
                assert [int(x) for x in outs[k][i]] == ref[k], (name, op, int(i))
    cs = D.cases(name, "fp28_k2mul")  # the same integers as the two dual products: bit-identical
    idx = cs.sample
    a0, a1, b0, b1 = cs.operands
    k0, k1 = _host_raw(hostmath, F, "fp28_k2mul", cs.operands, idx)
    assert np.array_equal(k0, _host_raw(hostmath, F, "fp28_mul2", (a0, b0, -a1, b1), idx)[0])
    assert np.array_equal(k1, _host_raw(hostmath, F, "fp28_mul2", (a0, b1, a1, b0), idx)[0])
    cs = D.cases(name, "fp28_reduce")
    idx = np.arange(cs.n_struct)
    got = _host_raw(hostmath, F, "fp28_reduce", cs.operands, idx)[0]
    assert ((D.values(got) - D.values(cs.operands[0][: cs.n_struct])) % F.p == 0).all()
    bound = 3 * F.p // 5
    assert D.low_limbs_normalized(got).all() and D.in_range(got, -bound, bound + 1).all(), name
    cs = D.cases(name, "fp28_normalize")
    idx = np.arange(cs.n_struct)
    got = _host_raw(hostmath, F, "fp28_normalize", cs.operands, idx)[0]
    assert np.array_equal(got.astype(np.int64), D.normalize_np(cs.operands[0][: cs.n_struct]))
    cs = D.cases(name, "fp28_from_fp")
    idx = np.arange(cs.n_struct)
    f = _host_raw(hostmath, F, "fp28_from_fp", cs.operands, idx)[0]
    a = np.array(D.sat_ints(cs.operands[0][: cs.n_struct]), dtype=object)
    assert ((D.values(f) * F.R - a * F.R28) % F.p == 0).all() and D.is_normalized(F, f).all()
    assert np.array_equal(_host_raw(hostmath, F, "fp28_to_fp", (f,), idx)[0], cs.operands[0][: cs.n_struct])
    cs = D.cases(name, "fp28_to_fp")
    idx = np.arange(cs.n_struct)
    got = _host_raw(hostmath, F, "fp28_to_fp", cs.operands, idx)[0]
    v = D.values(cs.operands[0][: cs.n_struct])
    assert np.array_equal(got, D.sat_array([int(x) for x in v * F.R * pow(F.R28, -1, F.p) % F.p], F.N))


def test_reference_held_products_through_the_host_carry_free_path(hostmath):
    """the products the reference's own constants fix (test_oracle_pinned.reference_held_products) through fp28_from_fp ->
    fp28_mul -> fp28_to_fp of the host build; tests/test_devmath_gpu.py runs the same table on the device"""
    from test_oracle_pinned import reference_held_products

    for a, b, ab in reference_held_products():
        out = ctypes.create_string_buffer(48)
        assert hostmath.hm_fp28_op(1, 1, a, b, None, None, out) == 0
        assert out.raw == ab


@pytest.mark.parametrize("gen, inc", [("gen_fp28_comba.py", "fp28_comba.inc"), ("gen_fp_comba.py", "fp_mul_comba.inc")])
def test_generators_print_the_committed_inc_files(gen, inc):
    """the .inc files are generated, never edited by hand: the generators reproduce them byte for byte"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen)], capture_output=True, check=True).stdout
    with open(os.path.join(ROOT, "mathlib_amd", "csrc", inc), "rb") as f:
        assert out == f.read()
