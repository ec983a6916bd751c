"""Inputs shared by the prepared-G2 tests (tests/test_g2_prepared_*.py): handles of m fixed G2 points -- with one point at
infinity and one point of E'(Fp2) outside the r-torsion where m allows -- batches of G1 points with infinities among them,
and the q_index forms (none, a permutation, a repeated index)."""
from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]


def g2_outside_subgroup(cp):
    Q = R._g2_some_point(cp, 3)
    assert R.g2_mul_unreduced(cp, Q, cp.r) is not None
    return Q


def handle_points(cp, m: int, tag: str):
    """m G2 points (pyref form; None = infinity): m = 1 one random point; m = 2 adds the point at infinity; m >= 3 also a
    point on the curve outside G2 (slot 2)"""
    d = R.Drbg("g2prep/handle/%s/%s/%d" % (cp.name, tag, m))
    qs = [R.random_g2(cp, d) for _ in range(m)]
    if m >= 2:
        qs[1] = None
    if m >= 3:
        qs[2] = g2_outside_subgroup(cp)
    return qs


def g2_bytes(cp, qs) -> bytes:
    return b"".join(R.g2_to_mont_bytes(cp, q) for q in qs)


def index_forms(m: int, ppp: int):
    """q_index forms valid for (m, ppp): None (needs ppp <= m), a permutation (reversed order), a repeated index"""
    forms = []
    if ppp <= m:
        forms.append(None)
        forms.append([m - 1 - j for j in range(ppp)])
    forms.append([(m - 1) if j % 2 == 0 else 0 for j in range(ppp)] if ppp > 1 else [m - 1])
    forms.append([0] * ppp)
    return forms


def g1_batch(cp, n: int, ppp: int, tag: str, inf_every: int = 7):
    """n * ppp G1 points from a handful of distinct random points (scalar multiples are slow in pyref), every inf_every-th
    one the point at infinity; returns (points in pyref form, bytes)"""
    d = R.Drbg("g2prep/g1/%s/%d/%d" % (tag, n, ppp))
    pool = [R.random_g1(cp, d) for _ in range(min(6, n * ppp))]
    pts = []
    for i in range(n * ppp):
        pts.append(None if (inf_every and d.below(inf_every) == 0) else pool[d.below(len(pool))])
    return pts, b"".join(R.g1_to_mont_bytes(cp, p) for p in pts)


def expand(qs, index, ppp: int, n: int):
    """the G2 argument of every pair, product after product"""
    idx = index if index is not None else list(range(ppp))
    return [qs[idx[j]] for _ in range(n) for j in range(ppp)]
