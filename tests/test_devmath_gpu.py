"""The device-only field multipliers on the GPU, at the bounds of their contracts.

mathlib_amd/csrc/fp_mul_comba.inc and fp28_comba.inc (generated gfx950 inline assembly) exist only under
__HIP_DEVICE_COMPILE__, so no CPU test can compile them.  tests/devmath/devmath.hip wraps them -- and the plain C++ around
them -- in elementwise kernels; this file builds it twice (as shipped, and with -DMLHIP_FP28_PORTABLE so that the device
runs fp28_mont / fp28_k2mul_portable), feeds both the operands of tests/devmath_cases.py (structured limb patterns at
every weight boundary, then random ones; 2^16 vectors per op and curve) and compares every output with Python integers.
Every comparison is exact integer equality or a range stated in fp28.h.  The chain is
    Python integers <-> host portable (tests/test_devmath_host.py) <-> device portable <-> device asm (here)."""
import ctypes

import numpy as np
import pytest

import devmath_cases as D

pytestmark = pytest.mark.gpu

CURVES = D.CURVES


def load_harness(path):
    lib = ctypes.CDLL(path)
    lib.dm_run.restype = ctypes.c_int
    lib.dm_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_size_t]
    lib.dm_fp28_is_asm.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def libs():
    """(the shipped form with the asm multipliers, the portable form)"""
    import torch

    assert torch.cuda.is_available(), "no GPU visible"
    asm, port = load_harness(D.build_harness(False)), load_harness(D.build_harness(True))
    assert asm.dm_fp28_is_asm() == 1 and port.dm_fp28_is_asm() == 0
    return asm, port


def run(lib, F, op, operands):
    """one launch of op over all vectors: (out, out2) as numpy arrays (uint32[n, N] or int32[n, L])"""
    import torch

    code = D.OPS[op]
    n = len(operands[0])
    in_w = F.N if (code < 16 or op == "fp28_from_fp") else F.L
    out_w = F.N if (code < 16 or op == "fp28_to_fp") else F.L
    dev = []
    for a in operands:  # the kernel reads n * in_w words of every operand and writes n * out_w
        assert a.shape == (n, in_w) and a.dtype in (np.int32, np.uint32), (op, a.shape, a.dtype)
        dev.append(torch.from_numpy(np.array(a).view(np.int32)).cuda())
    out = torch.zeros((n, out_w), dtype=torch.int32, device="cuda")
    out2 = torch.zeros((n, out_w), dtype=torch.int32, device="cuda")
    ptr = [t.data_ptr() for t in dev] + [None] * (4 - len(dev))
    torch.cuda.synchronize()
    rc = lib.dm_run(F.cid, code, *ptr, out.data_ptr(), out2.data_ptr(), n)
    assert rc == 0, (op, rc)
    view = np.uint32 if out_w == F.N else np.int32
    return out.cpu().numpy().view(view), out2.cpu().numpy().view(view)


def first_bad(mask):
    return int(np.flatnonzero(~mask)[0]) if not mask.all() else None


# ---- saturated form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_saturated_product_every_entry(libs, name):
    """fp_mul (out of line), fp_mul_i (inlined), fp_mul_inline (the portable CIOS on the device): a b R^-1 mod p for every
    vector, and the asm form equal to fp_mul_inline bit for bit (the claim at csrc/fp.h, above fp_mul_device)"""
    F = D.field(name)
    cs = D.cases(name, "fp_mul")
    a, b = (D.sat_ints(x) for x in cs.operands)
    rinv = pow(F.R, -1, F.p)
    want = D.sat_array([x * y * rinv % F.p for x, y in zip(a, b)], F.N)
    got = {op: run(libs[0], F, op, cs.operands)[0] for op in ("fp_mul", "fp_mul_i", "fp_mul_inline")}
    for op, g in got.items():
        assert first_bad((g == want).all(axis=1)) is None, (name, op)
    assert np.array_equal(got["fp_mul"], got["fp_mul_inline"]) and np.array_equal(got["fp_mul_i"], got["fp_mul_inline"])


@pytest.mark.parametrize("name", CURVES)
def test_saturated_square_and_dual_product(libs, name):
    F = D.field(name)
    rinv = pow(F.R, -1, F.p)
    cs = D.cases(name, "fp_sqr")
    a = D.sat_ints(cs.operands[0])
    got = run(libs[0], F, "fp_sqr", cs.operands)[0]
    assert first_bad((got == D.sat_array([x * x * rinv % F.p for x in a], F.N)).all(axis=1)) is None, name
    cs = D.cases(name, "fp_mul2")
    a, b, c, d = (D.sat_ints(x) for x in cs.operands)
    got = run(libs[0], F, "fp_mul2", cs.operands)[0]
    want = D.sat_array([(x * y + z * w) * rinv % F.p for x, y, z, w in zip(a, b, c, d)], F.N)
    assert first_bad((got == want).all(axis=1)) is None, name


@pytest.mark.parametrize("name", CURVES)
def test_saturated_add_sub_neg(libs, name):
    F = D.field(name)
    for op, f in (("fp_add", lambda x, y: (x + y) % F.p), ("fp_sub", lambda x, y: (x - y) % F.p)):
        cs = D.cases(name, op)
        a, b = (D.sat_ints(x) for x in cs.operands)
        got = run(libs[0], F, op, cs.operands)[0]
        assert first_bad((got == D.sat_array([f(x, y) for x, y in zip(a, b)], F.N)).all(axis=1)) is None, (name, op)
    cs = D.cases(name, "fp_neg")
    got = run(libs[0], F, "fp_neg", cs.operands)[0]
    assert first_bad((got == D.sat_array([-x % F.p for x in D.sat_ints(cs.operands[0])], F.N)).all(axis=1)) is None, name


@pytest.mark.parametrize("name", CURVES)
def test_divsteps_inversion(libs, hostmath, name):
    """fp_inv (modinv.h) on the device: a R -> a^-1 R, equal to pow(x, p - 2, p); x x^-1 = 1 through the device product;
    equal to the host twin on the structured list.  The inverse of 0 is 0, on the host and on the device (as with the
    Fermat inversion it replaced)."""
    F = D.field(name)
    cs = D.cases(name, "fp_inv")
    x = D.sat_ints(cs.operands[0])
    got = run(libs[0], F, "fp_inv", cs.operands)[0]
    want = D.sat_array([F.R * F.R * pow(v, F.p - 2, F.p) % F.p for v in x], F.N)
    assert first_bad((got == want).all(axis=1)) is None, name
    prod = run(libs[0], F, "fp_mul", (cs.operands[0], got))[0]
    one = D.sat_array([F.R % F.p if v else 0 for v in x], F.N)
    assert np.array_equal(prod, one)
    assert x[0] == 0 and not got[0].any()
    buf = ctypes.create_string_buffer(4 * F.N)
    for i in range(cs.n_struct):
        assert hostmath.hm_fp_op(F.cid, 9, cs.operands[0][i].tobytes(), None, buf) == 0
        assert buf.raw == got[i].tobytes(), (name, i)


def test_reference_held_products_through_every_multiplier(libs):
    """The only products the REFERENCE itself fixes (test_oracle_pinned.reference_held_products: the Montgomery-form SWU
    constants of its BLS12-381 driver, 1 * 1 = 1 and x * 1 = x) through every saturated entry of the harness and through
    the carry-free path fp28_from_fp -> fp28_mul -> fp28_to_fp in both forms: byte equality with the held result.  The
    k_fp_mul run of the same table stays in tests/test_gpu_parity.py::test_fp_mul_reference_held_products."""
    from test_oracle_pinned import reference_held_products

    F = D.field("BLS12-381")
    table = reference_held_products()
    a, b, ab = (np.frombuffer(b"".join(t[k] for t in table), dtype="<u4").reshape(-1, F.N).copy() for k in range(3))
    zero = np.zeros_like(a)
    for op in ("fp_mul", "fp_mul_i", "fp_mul_inline"):
        assert run(libs[0], F, op, (a, b))[0].tobytes() == ab.tobytes(), op
    assert run(libs[0], F, "fp_mul2", (a, b, zero, zero))[0].tobytes() == ab.tobytes()  # a b + 0 0
    assert run(libs[0], F, "fp_mul2", (zero, b, b, a))[0].tobytes() == ab.tobytes()  # 0 b + b a
    sq = [i for i, t in enumerate(table) if t[0] == t[1]]  # 1 * 1 = 1
    assert sq and run(libs[0], F, "fp_sqr", (a[sq],))[0].tobytes() == ab[sq].tobytes()
    for lib in libs:
        fa, fb = (run(lib, F, "fp28_from_fp", (x,))[0] for x in (a, b))
        prod = run(lib, F, "fp28_mul", (fa, fb))[0]
        assert run(lib, F, "fp28_to_fp", (prod,))[0].tobytes() == ab.tobytes()
        dual = run(lib, F, "fp28_mul2", (fa, fb, fb, fa))[0]  # a b + b a = 2 a b
        two_ab = run(libs[0], F, "fp_add", (ab, ab))[0]
        assert run(lib, F, "fp28_to_fp", (dual,))[0].tobytes() == two_ab.tobytes()


# ---- carry-free form -------------------------------------------------------------------------------------------------
def check_products(F, op, cs, outs):
    """residue and normalisation of every output of a product op, and the structured sample against the transcription"""
    vals = [D.values(a) for a in cs.operands]
    for k, want in enumerate(D.product_integers(op, vals)):
        got = D.values(outs[k])
        diff = (got * F.R28 - want) % F.p
        assert first_bad(diff == 0) is None, (F.name, op, k, "residue")
        assert first_bad(D.is_normalized(F, outs[k])) is None, (F.name, op, k, "not normalized")
    for i in cs.sample:
        v = [[int(x) for x in o[i]] for o in cs.operands]
        ref = D.transcription(F, op, v)
        for k in range(len(ref)):
            assert [int(x) for x in outs[k][i]] == ref[k], (F.name, op, int(i), k)


@pytest.mark.parametrize("op", ["fp28_mul", "fp28_sqr", "fp28_mul2", "fp28_k2mul"])
@pytest.mark.parametrize("name", CURVES)
def test_fp28_products(libs, name, op):
    """Both forms of every carry-free product: the residue a b / R28 (resp. a^2, a b + c d, the two k2mul components) and
    the normalisation of fp28.h for every vector, the structured sample limb for limb against the Python transcription of
    fp28_mont, and the asm form equal to the portable form limb for limb for every vector ("same arithmetic")."""
    F = D.field(name)
    cs = D.cases(name, op)
    nout = 2 if op == "fp28_k2mul" else 1
    asm = run(libs[0], F, op, cs.operands)[:nout]
    port = run(libs[1], F, op, cs.operands)[:nout]
    check_products(F, op, cs, port)
    same = all(np.array_equal(asm[k], port[k]) for k in range(nout))
    if not same:  # tell a wrong product (fails here) from a right one in another representation (fails below)
        check_products(F, op, cs, asm)
    for k in range(nout):
        assert first_bad((asm[k] == port[k]).all(axis=1)) is None, (name, op, k, "asm != portable")
    if op == "fp28_k2mul":  # fp28.h: bit-identical to fp28_mul2(a0, b0, -a1, b1) and fp28_mul2(a0, b1, a1, b0)
        a0, a1, b0, b1 = cs.operands
        for lib in libs:
            c0 = run(lib, F, "fp28_mul2", (a0, b0, -a1, b1))[0]
            c1 = run(lib, F, "fp28_mul2", (a0, b1, a1, b0))[0]
            assert np.array_equal(c0, asm[0]) and np.array_equal(c1, asm[1]), name


@pytest.mark.parametrize("name", CURVES)
def test_fp28_reduce_and_normalize(libs, name):
    """fp28_reduce on the inputs of test_host_math.py::test_fp28_reduce_range (values up to 600 p, un-normalized limbs up
    to weight 8), on every curve: the same residue, limbs 0..L-2 in [0, 2^28), |value| < 0.6 p.  fp28_normalize: the same
    VALUE, limbs 0..L-2 in [0, 2^28)."""
    F = D.field(name)
    cs = D.cases(name, "fp28_reduce")
    vin = D.values(cs.operands[0])
    for lib in libs:
        got = run(lib, F, "fp28_reduce", cs.operands)[0]
        assert first_bad((D.values(got) - vin) % F.p == 0) is None, name
        assert first_bad(D.low_limbs_normalized(got)) is None, name
        bound = 3 * F.p // 5  # |v| < 0.6 p  <=>  |v| <= floor(0.6 p)
        assert first_bad(D.in_range(got, -bound, bound + 1)) is None, name
    cs = D.cases(name, "fp28_normalize")
    got = run(libs[0], F, "fp28_normalize", cs.operands)[0]
    assert np.array_equal(got.astype(np.int64), D.normalize_np(cs.operands[0]))
    assert first_bad(D.values(got) == D.values(cs.operands[0])) is None and first_bad(D.low_limbs_normalized(got)) is None


@pytest.mark.parametrize("name", CURVES)
def test_fp28_boundary_conversions(libs, name):
    """fp28_from_fp: x R -> x R28, normalized; fp28_to_fp after it is the identity on canonical values; fp28_to_fp of
    inputs of weight up to 8 (what its comment allows) is the canonical residue.  Both forms."""
    F = D.field(name)
    cs = D.cases(name, "fp28_from_fp")
    a = np.array(D.sat_ints(cs.operands[0]), dtype=object)
    w8 = D.cases(name, "fp28_to_fp")
    v8 = D.values(w8.operands[0])
    want8 = D.sat_array([int(v) for v in v8 * F.R * pow(F.R28, -1, F.p) % F.p], F.N)
    res = []
    for lib in libs:
        f = run(lib, F, "fp28_from_fp", cs.operands)[0]
        assert first_bad((D.values(f) * F.R - a * F.R28) % F.p == 0) is None, name
        assert first_bad(D.is_normalized(F, f)) is None, name
        back = run(lib, F, "fp28_to_fp", (f,))[0]
        assert first_bad((back == cs.operands[0]).all(axis=1)) is None, name
        got8 = run(lib, F, "fp28_to_fp", w8.operands)[0]
        assert first_bad((got8 == want8).all(axis=1)) is None, name
        res.append(f)
    assert np.array_equal(res[0], res[1])
