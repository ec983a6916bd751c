"""Inputs of the G2 bucket-route tests of the batched MSM (tests/test_msm_batch_bucket_g2_host.py,
tests/test_msm_batch_bucket_g2_gpu.py): the G2 counterpart of tests/msm_batch_bucket_cases.py.  The lane-pair kernels of
mathlib_amd/csrc/msm_batch_bucket.h cut a scalar into 6-bit signed windows (32 buckets, one per lane pair of a wave), so the
special scalars sit at that width's boundaries: 31 | 32 | 33 (32 is the largest positive digit and lands in the last lane
pair, the first one "beyond" which the reduction must see infinity; 33 is -31 with a carry) and 63 | 64.  Expected bytes:
msm_batch_cases.expected (cref.msm per segment)."""
import functools
import random

from msm_batch_bucket_cases import CURVES, FORCED_MIN, FORCED_SLICE, MIXED_LENGTHS, all_ones_scalar, curve  # noqa: F401
from msm_batch_cases import edge_segments, neg_point, point_bytes, random_segments, sc
from oracle import cref
from oracle import pyref as R
from point_sum_cases import outside_subgroup_point

GROUP = 2
SPECIAL = [0, 1, 31, 32, 33, 63, 64]  # + 2^256 - 1, r - 1, r, r + 1 per curve


def _points(cp, n: int, salt: int):
    ps = point_bytes(cp, GROUP)
    raw = cref.gen_points(cp.curve_id, GROUP, 0xB0C4E7 + salt, 0x62 + n, n)
    return [raw[i * ps : (i + 1) * ps] for i in range(n)]


@functools.lru_cache(maxsize=None)
def cases(name: str):
    """[(case name, points, scalars, lengths)] of one curve, G2"""
    cp = curve(name)
    rnd = random.Random("bucket-g2-cases/" + name)
    r = cp.r
    ps = point_bytes(cp, GROUP)
    inf = bytes(ps)
    out = []

    def add(case, pts, scs, lengths):
        assert len(pts) == len(scs) == sum(lengths)
        out.append((case, b"".join(pts), b"".join(sc(v) for v in scs), list(lengths)))

    for pad in (9, 16):  # 16: with slices of 16 the degenerate pairs straddle slice boundaries
        p, s, l = edge_segments(cp, GROUP, "bucket-g2-edge/%s/%d" % (name, pad), pad=pad)
        out.append(("edge_pad%d" % pad, p, s, l))
    P = _points(cp, 44, 1)
    special = SPECIAL + [(1 << 256) - 1, r - 1, r, r + 1]
    pts, scs = [], []
    for i, v in enumerate(special):  # each special scalar between two random pairs
        pts += [P[2 * i], P[2 * i + 1]]
        scs += [rnd.randrange(r), v]
    # ... then 8 random pairs, and a segment of the special scalars alone (11 pairs: one slice)
    add("special_scalars", pts + P[22:41], scs + [rnd.randrange(r) for _ in range(8)] + special, [30, 11])
    ones = all_ones_scalar(cp)
    add("all_ones_windows", P[:20], [ones] * 10 + [rnd.randrange(r) for _ in range(10)], [20])
    s = rnd.randrange(1, r)
    add("one_scalar_40_points", P[:40], [s] * 40, [40])
    add("one_pair_40_times", [P[3]] * 40, [s] * 40, [40])
    add("cancelling_pairs", [P[5], neg_point(cp, GROUP, P[5])] * 20, [s] * 40, [40])
    add("only_infinities", [inf] * 20 + [P[7]] * 12 + [inf] * 16, [rnd.randrange(r) for _ in range(48)], [20, 28])
    q = R.g2_to_mont_bytes(cp, outside_subgroup_point(name, GROUP))  # exists on the twist of all three curves
    pts = list(P[:30])
    pts[4] = pts[15] = pts[16] = pts[29] = q  # inside a slice, at both ends of a slice boundary, last of the segment
    add("outside_subgroup", pts, [rnd.randrange(r) for _ in range(30)], [30])
    p, s, l = random_segments(cp, GROUP, MIXED_LENGTHS, "bucket-g2-mixed/" + name)
    out.append(("mixed", p, s, l))
    return out
