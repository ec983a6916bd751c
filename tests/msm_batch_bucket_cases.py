"""Inputs of the bucket-route tests of the batched MSM (tests/test_msm_batch_bucket_host.py,
tests/test_msm_batch_bucket_gpu.py): G1 batches whose long segments hold every input the bucket kernels of
mathlib_amd/csrc/msm_batch_bucket.h may not assume away -- infinities, zero and unreduced scalars, one bucket taking a whole
slice, the same pair again and again (the doubling branch), P next to -P, a 2-torsion point, a point outside the prime-order
subgroup -- inside one slice and across slice boundaries.  Expected bytes: msm_batch_cases.expected (cref.msm per segment)."""
import functools
import random

from msm_batch_cases import edge_segments, neg_point, point_bytes, random_segments, sc
from oracle import cref
from oracle import pyref as R
from point_sum_cases import outside_subgroup_point

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
FORCED_MIN, FORCED_SLICE = 9, 16  # MLHIP_MSM_BATCH_BUCKET_MIN / _SLICE of the forced runs: several slices out of 40 pairs
MIXED_LENGTHS = [0, 40, 3, 0, 17, 9, 8, 200, 1, 0]


def curve(name: str):
    return R.CURVES[name]


def _points(cp, n: int, salt: int):
    ps = point_bytes(cp, 1)
    raw = cref.gen_points(cp.curve_id, 1, 0xB0C4E7 + salt, 0x51 + n, n)
    return [raw[i * ps : (i + 1) * ps] for i in range(n)]


def all_ones_scalar(cp) -> int:
    """every 7-bit (6-bit) window below the top one all ones: window 0 is -1 with a carry, every later one 2^width with a
    carry = digit 0 ("minus zero") with a carry, up to the top window, which takes the last carry"""
    return (1 << (cp.r.bit_length() - 1)) - 1


@functools.lru_cache(maxsize=None)
def cases(name: str):
    """[(case name, points, scalars, lengths)] of one curve, G1"""
    cp = curve(name)
    rnd = random.Random("bucket-cases/" + name)
    r = cp.r
    ps = point_bytes(cp, 1)
    inf = bytes(ps)
    out = []

    def add(case, pts, scs, lengths):
        assert len(pts) == len(scs) == sum(lengths)
        out.append((case, b"".join(pts), b"".join(sc(v) for v in scs), list(lengths)))

    for pad in (9, 16):  # 16: with slices of 16 the degenerate pairs straddle slice boundaries
        p, s, l = edge_segments(cp, 1, "bucket-edge/%s/%d" % (name, pad), pad=pad)
        out.append(("edge_pad%d" % pad, p, s, l))
    P = _points(cp, 72, 1)
    special = [0, 1, 64, 65, (1 << 256) - 1, r - 1, r, r + 1]
    pts, scs = [], []
    for i, v in enumerate(special):  # each special scalar between two random pairs
        pts += [P[2 * i], P[2 * i + 1]]
        scs += [rnd.randrange(r), v]
    # ... then 8 random pairs, and a segment of the special scalars alone (8 pairs: Straus chunks)
    add("special_scalars", pts + P[16:32], scs + [rnd.randrange(r) for _ in range(8)] + special, [24, 8])
    ones = all_ones_scalar(cp)
    add("all_ones_windows", P[:20], [ones] * 10 + [rnd.randrange(r) for _ in range(10)], [20])
    s = rnd.randrange(1, r)
    add("one_scalar_70_points", P[:70], [s] * 70, [70])
    add("one_pair_70_times", [P[3]] * 70, [s] * 70, [70])
    add("cancelling_pairs", [P[5], neg_point(cp, 1, P[5])] * 35, [s] * 70, [70])
    add("only_infinities", [inf] * 20 + [P[7]] * 12 + [inf] * 16, [rnd.randrange(r) for _ in range(48)], [20, 28])
    if name == "BLS12-377":
        tor = R.g1_to_mont_bytes(cp, (cp.p - 1, 0))  # (-1, 0): y = 0, so P + P = infinity and -P = P
        pts = [tor, P[0], tor, tor, P[1], tor] * 4
        add("two_torsion", pts, [rnd.randrange(r) for _ in range(24)], [24])
        add("two_torsion_same_scalar", [tor] * 17 + [P[2]], [5] * 17 + [rnd.randrange(r)], [18])
    x = outside_subgroup_point(name, 1)
    if x is not None:
        q = R.g1_to_mont_bytes(cp, x)
        pts = list(P[:30])
        pts[4] = pts[15] = pts[16] = pts[29] = q
        add("outside_subgroup", pts, [rnd.randrange(r) for _ in range(30)], [30])
    p, s, l = random_segments(cp, 1, MIXED_LENGTHS, "bucket-mixed/" + name)
    out.append(("mixed", p, s, l))
    return out
