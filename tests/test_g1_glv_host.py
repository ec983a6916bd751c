"""The GLV lattice split of BN254 G1 behind the two promised routes (MLHIP_GROUP_SUBGROUP on mlhip_scalar_mul*,
MLHIP_CURVE_SUBGROUP_POINTS on mlhip_msm_batch*) without a GPU.  The device code of mathlib_amd/csrc/msm_scalar_mul_endo.h and
msm_batch_endo.h compiled for the CPU (tests/hostmath_glv): the compiled constants against Python integers and
oracle/pyref.py's multiplication, g1_glv_split against the same split in Python integers on every boundary it has, the chain
against R.g1_mul, the chunk body against cref.msm of every segment, and what chain and chunk give for a point OFF the curve
(the value that makes the route observable on the GPU)."""
import ctypes
import random

import pytest

from g1_glv_cases import (CHUNKS, CP, LAM, T, basis, beta, glv_edge_segments, harness, host_batch, host_mul, host_split,
                          scalar_rows, special_scalars, split)
from msm_batch_cases import edge_segments, expected, random_segments
from oracle import pyref as R
from point_sum_cases import distinct_points


@pytest.fixture(scope="module")
def glv():
    return harness()


def test_which_curves_have_the_lattice_split(glv):
    """BN254 alone, under a trait of its own: ScalarMulEndo<C, true> (s = a + b x^2 exists) keeps its values"""
    assert [glv.glv_available(c) for c in (0, 1, 2)] == [1, 2, 2]


def test_compiled_constants(glv):
    beta_b, lam_b, g1, g2 = (ctypes.create_string_buffer(32) for _ in range(4))
    basis_b = ctypes.create_string_buffer(64)
    neg = (ctypes.c_int * 4)()
    glv.glv_constants(beta_b, lam_b, basis_b, neg, g1, g2)
    r, p = CP.r, CP.p
    lam = int.from_bytes(lam_b.raw, "little")
    assert lam == LAM and (lam * lam + lam + 1) % r == 0
    assert int.from_bytes(beta_b.raw, "little") == beta() * CP.R % p
    mag = [int.from_bytes(basis_b.raw[16 * i : 16 * i + 16], "little") for i in range(4)]
    a1, b1, a2, b2 = (-m if n else m for m, n in zip(mag, neg))
    assert ((a1, b1), (a2, b2)) == basis()
    assert (a1 + b1 * lam) % r == 0 and (a2 + b2 * lam) % r == 0 and a1 * b2 - b1 * a2 == r
    assert int.from_bytes(g1.raw, "little") == (abs(b2) << 256) // r and int.from_bytes(g2.raw, "little") == (abs(b1) << 256) // r
    # (beta x, y) = [lambda]P through the compiled beta: random points, the generator, infinity
    d = R.Drbg("g1_glv/phi")
    out = ctypes.create_string_buffer(64)
    for P in [R.random_g1(CP, d) for _ in range(3)] + [CP.g1, None]:
        glv.glv_phi(R.g1_to_mont_bytes(CP, P), out)
        assert out.raw == R.g1_to_mont_bytes(CP, R.g1_mul(CP, P, LAM))


def test_split_matches_python_integers(glv):
    """k1 + k2 lambda = s mod r, |k1|, |k2| < 2^128 (the contract) and < 3/4 (A + 2 B) < 2^127 (what the header proves), equal to
    the same fixed-point split in Python; all four sign combinations occur"""
    (a1, b1), (a2, b2) = basis()
    bound = 3 * (a1 + 2 * a2) // 4 + 1
    assert bound < 1 << 127
    rnd = random.Random("g1_glv/split")
    rows = [(raw, k, mont) for mont in (0, 1) for raw, k in scalar_rows(mont)]
    rows += [(rnd.getrandbits(256).to_bytes(32, "little"), None, mont) for mont in (0, 1) for _ in range(2000)]
    signs = set()
    for raw, k, mont in rows:
        k1, k2, canon = host_split(glv, raw, mont)
        if k is None:
            v = int.from_bytes(raw, "little")
            k = (v * pow(1 << 256, -1, CP.r) if mont else v) % CP.r
        assert canon == k, (raw.hex(), mont)
        assert (k1, k2) == split(k), (hex(k), mont)
        assert (k1 + k2 * LAM - k) % CP.r == 0 and abs(k1) < bound and abs(k2) < bound, (hex(k), mont)
        signs.add((k1 < 0, k2 < 0))
    assert len(signs) == 4
    assert split(0) == (0, 0) and split(1) == (1, 0) and split(LAM) == (0, 1) and split(CP.r - LAM) == (0, -1)


def test_chain_matches_g1_mul(glv):
    P = R.random_g1(CP, R.Drbg("g1_glv/chain"))
    for mont in (0, 1):
        for i, (raw, k) in enumerate(scalar_rows(mont)):
            assert host_mul(glv, P, raw, mont) == R.g1_to_mont_bytes(CP, R.g1_mul(CP, P, k)), (hex(k), mont)
            if i < 6:
                assert host_mul(glv, None, raw, mont) == bytes(64)
    for s in (0, CP.r):
        assert host_mul(glv, P, s.to_bytes(32, "little"), 0) == bytes(64)
    assert host_mul(glv, P, LAM.to_bytes(32, "little"), 0) == R.g1_to_mont_bytes(CP, (beta() * P[0] % CP.p, P[1]))


def test_chain_off_the_curve_is_the_endomorphism_not_the_product(glv):
    """s = lambda is k1 = 0, k2 = 1: the chain returns exactly (beta x, y), which is not [lambda]T for T = (1, 3) on
    y^2 = x^3 + 8"""
    assert (T[1] ** 2 - T[0] ** 3 - CP.b) % CP.p != 0 and (T[1] ** 2 - T[0] ** 3 - 8) % CP.p == 0
    got = host_mul(glv, T, LAM.to_bytes(32, "little"), 0)
    assert got == R.g1_to_mont_bytes(CP, (beta(), 3))
    assert got != R.g1_to_mont_bytes(CP, R.g1_mul(CP, T, LAM))


def test_segments_of_every_length_and_chunk(glv):
    """lengths 0, 1, P - 1, P, P + 1, 17 and 64 over uniform 256-bit scalars (mostly unreduced), both scalar forms"""
    for P in CHUNKS:
        lengths = [0, 1, max(P - 1, 0), P, P + 1, 3, 0, 17, 64]
        pts, scs, lengths = random_segments(CP, 1, lengths, "g1-glv-host/%d" % P)
        for mont in (False, True):
            rc, got = host_batch(glv, P, pts, scs, lengths, mont)
            assert rc == 0 and got == expected(CP, 1, pts, scs, lengths, mont), (P, mont)
    rc, got = host_batch(glv, 3, b"", b"", [0], False)
    assert rc == -5


def test_scalars_on_the_boundaries_of_the_split_in_chunks(glv):
    base = distinct_points("BN254", 1, 300)
    for mont in (0, 1):
        rows = scalar_rows(mont)
        pts = [base[i] for i in range(len(rows))]
        pts[len(rows) // 3] = None
        lengths, left, cyc = [], len(rows), 0
        while left:
            lengths.append(min(left, (1, 2, 3, 5, 8, 4, 7)[cyc % 7]))
            left -= lengths[-1]
            cyc += 1
        raw_p = b"".join(R.g1_to_mont_bytes(CP, p) for p in pts)
        raw_s = b"".join(raw for raw, _ in rows)
        exp = expected(CP, 1, raw_p, raw_s, lengths, bool(mont))
        for P in CHUNKS:
            rc, got = host_batch(glv, P, raw_p, raw_s, lengths, bool(mont))
            assert rc == 0 and got == exp, (mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])


def test_degenerate_pairs_inside_one_chunk(glv):
    for make in (lambda seed, pad: edge_segments(CP, 1, seed, pad), glv_edge_segments):
        for pad in (0, 1, 3):
            pts, scs, lengths = make("g1-glv-host-edge", pad)
            for mont in (False, True):
                exp = expected(CP, 1, pts, scs, lengths, mont)
                for P in CHUNKS:
                    rc, got = host_batch(glv, P, pts, scs, lengths, mont)
                    assert rc == 0 and got == exp, (pad, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])
    # the new cases test what they claim: the cancellations are the point at infinity, the meeting pairs are [2 d]Q
    pts, scs, lengths = glv_edge_segments("g1-glv-host-edge", 0)
    exp = expected(CP, 1, pts, scs, lengths, False)
    assert exp[2] == exp[3] == exp[8] == bytes(64)
    d = int.from_bytes(scs[32:64], "little")
    Q = R.g1_mul(CP, distinct_points("BN254", 1, 300)[7], LAM)
    assert pts[64:128] == R.g1_to_mont_bytes(CP, Q)
    assert exp[0] == exp[1] == R.g1_to_mont_bytes(CP, R.g1_mul(CP, Q, 2 * d))


def test_chunk_off_the_curve_is_the_endomorphism_not_the_product(glv):
    """T with s = lambda alone in a segment: every chunk length returns (beta, 3); its neighbours do not see it"""
    base = distinct_points("BN254", 1, 300)
    pts = b"".join(R.g1_to_mont_bytes(CP, p) for p in (base[1], T, base[2]))
    scs = b"".join(v.to_bytes(32, "little") for v in (5, LAM, 7))
    want = [R.g1_to_mont_bytes(CP, p) for p in (R.g1_mul(CP, base[1], 5), (beta(), 3), R.g1_mul(CP, base[2], 7))]
    assert want[1] != R.g1_to_mont_bytes(CP, R.g1_mul(CP, T, LAM))
    for P in CHUNKS:
        rc, got = host_batch(glv, P, pts, scs, [1, 1, 1], False)
        assert rc == 0 and got == want, P
