"""Inputs and expected outputs of the point-sum tests (tests/test_point_sum_host.py, tests/test_point_sum_gpu.py): lists
that drive every branch of the complete mixed addition -- a repeated point (doubling), P, -P pairs (infinity), points at
infinity at the first, middle and last position, an all-infinity list, a list that sums to infinity, and a point of the
curve outside the prime-order subgroup -- with oracle.pyref's affine additions as the expected bytes."""
import functools

from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
SIZES = (1, 2, 3, 33, 64 * 3 + 1)  # the lengths the compositions below are built at
COMPOSITIONS = ["repeated", "pairs", "infinities", "all_infinity", "sums_to_infinity", "outside_subgroup"]


def curve(name: str):
    return R.CURVES[name]


def point_bytes(cp, group: int) -> int:
    return 2 * group * cp.fp_bytes


def ops(cp, group: int):
    """(add, neg, to_bytes, from_bytes) of the group in oracle.pyref"""
    if group == 1:
        return (lambda a, b: R.g1_add(cp, a, b), lambda a: R.g1_neg(cp, a), lambda a: R.g1_to_mont_bytes(cp, a),
                lambda b: R.g1_from_mont_bytes(cp, b))
    return (lambda a, b: R.g2_add(cp, a, b), lambda a: R.g2_neg(cp, a), lambda a: R.g2_to_mont_bytes(cp, a),
            lambda b: R.g2_from_mont_bytes(cp, b))


@functools.lru_cache(maxsize=None)
def distinct_points(name: str, group: int, n: int = 200):
    """P_0, P_0 + Q, P_0 + 2 Q, ...: n distinct points of the prime-order subgroup"""
    cp = curve(name)
    add = ops(cp, group)[0]
    d = R.Drbg("point-sum/%s/%d" % (name, group))
    rnd = R.random_g1 if group == 1 else R.random_g2
    p, q = rnd(cp, d), rnd(cp, d)
    out = []
    for _ in range(n):
        out.append(p)
        p = add(p, q)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def outside_subgroup_point(name: str, group: int):
    """a point of the curve (G2: of the twist) that [r] does not send to infinity; None where the group has cofactor 1"""
    cp = curve(name)
    if group == 1:
        if cp.family != "BLS12":
            return None  # BN254: E(Fp) has prime order
        x = 2
        while True:
            y = R.fp_sqrt((x**3 + cp.b) % cp.p, cp.p)
            if y is not None and R.g1_mul_unreduced(cp, (x, y), cp.r) is not None:
                return (x, y)
            x += 1
    k = 3
    while True:
        q = R._g2_some_point(cp, k)
        if R.g2_mul_unreduced(cp, q, cp.r) is not None:
            return q
        k += 1


def composition(name: str, group: int, kind: str, n: int):
    """a list of n points (None = infinity) of the given kind, or None where the kind does not exist (no point outside the
    subgroup on BN254's G1)"""
    cp = curve(name)
    add, neg, _, _ = ops(cp, group)
    pts = distinct_points(name, group)
    if kind == "repeated":
        return [pts[0]] * n
    if kind == "pairs":
        return [pts[1] if i % 2 == 0 else neg(pts[1]) for i in range(n)]
    if kind == "infinities":
        out = list(pts[2 : 2 + n])
        for i in (0, n // 2, n - 1):
            out[i] = None
        return out
    if kind == "all_infinity":
        return [None] * n
    if kind == "sums_to_infinity":
        out = list(pts[3 : 3 + n - 1])
        total = None
        for p in out:
            total = add(total, p)
        return out + [neg(total)]
    if kind == "outside_subgroup":
        x = outside_subgroup_point(name, group)
        if x is None:
            return None
        out = list(pts[4 : 4 + n])
        out[n // 2] = x
        return out
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case_bytes(name: str, group: int, kind: str, n: int):
    """(the list in the C-ABI layout, its expected sum), computed once per session; None where the kind does not exist"""
    pts = composition(name, group, kind, n)
    if pts is None:
        return None
    cp = curve(name)
    return pack(cp, group, pts), expected(cp, group, pts)


def pack(cp, group: int, points) -> bytes:
    return b"".join(ops(cp, group)[2](p) for p in points)


def expected(cp, group: int, points) -> bytes:
    """the affine sum in the C-ABI layout, by oracle.pyref's additions in list order"""
    add, _, to_bytes, _ = ops(cp, group)
    total = None
    for p in points:
        total = add(total, p)
    return to_bytes(total)
