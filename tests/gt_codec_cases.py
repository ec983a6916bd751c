"""Shared by the gt_codec tests (host, GPU, mirrors): per curve, Fp12 values inside and outside Gt and malformed wire
encodings, all computed once with oracle/pyref.py.  Every value's membership is confirmed here by the definition -- f^r == 1
(f12_pow), for 0 by f == 0 -- so the expected statuses do not rest on the criterion under test."""
import functools
from collections import namedtuple

from oracle import pyref as R

CURVES = ("BN254", "BLS12-381", "BLS12-377")
OK, MALFORMED, NOT_MEMBER = 0, 1, 3

Value = namedtuple("Value", "label f member")  # f: pyref's w-basis tuple
Wire = namedtuple("Wire", "label wire status f")  # status with the check; f: the value behind a well-formed encoding, else None


def _easy_part(cp, t):
    """t^((p^6 - 1)(p^2 + 1)): in the cyclotomic subgroup, in general not of order r"""
    T = R.tower(cp)
    u = T.f12_mul(T.f12_conj(t), T.f12_inv(t))
    return T.f12_mul(T.f12_frob(u, 2), u)


@functools.lru_cache(maxsize=None)
def values(name):
    cp = R.CURVES[name]
    T = R.tower(cp)
    d = R.Drbg("gt_codec/" + name)
    P, Q = R.random_g1(cp, d), R.random_g2(cp, d)
    raw = R.miller_loop(cp, [(P, Q)])
    m = R.final_exp(cp, raw)
    m2 = R.pairing(cp, R.random_g1(cp, d), R.random_g2(cp, d))
    rnd = tuple((d.below(cp.p), d.below(cp.p)) for _ in range(6))
    e = _easy_part(cp, rnd)
    zero = tuple(T.f2_zero for _ in range(6))
    flipped = list(m)
    flipped[3] = (flipped[3][0] ^ 1, flipped[3][1])
    assert flipped[3][0] < cp.p
    members = [
        ("pairing", m),
        ("one", T.f12_one),
        ("conj", T.f12_conj(m)),
        ("square", T.f12_sqr(m)),
        ("product", T.f12_mul(m, m2)),
    ]
    outside = [
        ("zero", zero),
        ("minus-one", T.f12_neg(T.f12_one)),
        ("random", rnd),
        ("miller", raw),
        ("easy-part", e),
        ("member-times-easy-part", T.f12_mul(m, e)),
        ("bit-flip", tuple(flipped)),
    ]
    out = []
    for label, f in members:
        assert T.f12_is_one(T.f12_pow(f, cp.r)), (name, label)
        out.append(Value(label, f, True))
    for label, f in outside:
        if label == "zero":
            assert all(T.f2_is_zero(c) for c in f)
        else:
            assert not T.f12_is_one(T.f12_pow(f, cp.r)), (name, label)
        out.append(Value(label, f, False))
    # the easy-part output is what condition (ii) exists for: it passes (i)
    assert T.f12_mul(T.f12_frob(T.f12_frob(e, 2), 2), e) == T.f12_frob(e, 2)
    return tuple(out)


def _replace(cp, wire, k, coord):
    n = cp.fp_bytes
    return wire[: k * n] + coord + wire[(k + 1) * n :]


@functools.lru_cache(maxsize=None)
def wires(name):
    """every value's encoding, then the malformed ones"""
    cp = R.CURVES[name]
    vals = values(name)
    out = [Wire(v.label, R.gt_wire_bytes(cp, v.f), OK if v.member else NOT_MEMBER, v.f) for v in vals]
    member = R.gt_wire_bytes(cp, vals[0].f)
    outside = R.gt_wire_bytes(cp, vals[7].f)  # the random value
    p = cp.p.to_bytes(cp.fp_bytes, "big")
    ones = b"\xff" * cp.fp_bytes
    out += [
        Wire("first-coordinate-p", _replace(cp, member, 0, p), MALFORMED, None),
        Wire("last-coordinate-p", _replace(cp, member, 11, p), MALFORMED, None),
        Wire("all-ones-coordinate", _replace(cp, member, 5, ones), MALFORMED, None),
        Wire("outside-and-malformed", _replace(cp, outside, 7, p), MALFORMED, None),
    ]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def inverse_bytes(name):
    """{label: in-memory bytes of pyref's f12_inv(f)}; the inverse of 0 is 0 (gnark's E12.Inverse; pyref's modular inverse
    refuses 0, so that one value is written down here)"""
    cp = R.CURVES[name]
    T = R.tower(cp)
    return {v.label: R.gt_to_mont_bytes(cp, v.f if v.label == "zero" else T.f12_inv(v.f)) for v in values(name)}
