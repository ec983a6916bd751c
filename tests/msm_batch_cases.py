"""Inputs and expected outputs of the batched MSM tests (tests/test_msm_batch_host.py, tests/test_msm_batch_gpu.py):
segments of mixed lengths and the edge cases that interleaving the pairs of one chunk makes reachable, with cref.msm of
every segment as the expected bytes."""
import random

from oracle import cref
from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]


def point_bytes(cp, group: int) -> int:
    return 2 * group * cp.fp_bytes


def neg_point(cp, group: int, raw: bytes) -> bytes:
    """-P in the C-ABI layout (Montgomery coordinates; infinity = all zero stays so)"""
    n = cp.fp_bytes
    if not any(raw):
        return raw
    out = bytearray(raw)
    for i in range(group, 2 * group):  # the y coordinate's Fp components
        v = int.from_bytes(raw[i * n : (i + 1) * n], "little")
        out[i * n : (i + 1) * n] = ((cp.p - v) % cp.p).to_bytes(n, "little")
    return bytes(out)


def sc(v: int) -> bytes:
    return (v % (1 << 256)).to_bytes(32, "little")


def random_segments(cp, group: int, lengths, seed: str):
    """segments of the given lengths over distinct points; scalars uniform 256-bit integers (mostly >= r: not canonical)"""
    rnd = random.Random(seed)
    n = sum(lengths)
    pts = cref.gen_points(cp.curve_id, group, 0x5EED + len(seed), 0x1234567 + n, max(n, 1))[: n * point_bytes(cp, group)]
    scs = b"".join(sc(rnd.getrandbits(256)) for _ in range(n))
    return pts, scs, list(lengths)


def edge_segments(cp, group: int, seed: str, pad: int = 0):
    """segments that put degenerate pairs side by side inside one chunk (any P >= 2): points at infinity, zero scalars,
    scalars >= r, the same (P, s) repeated (the accumulator meets its own table entry: the doubling branch), (P, s) next to
    (-P, s) and (P, s) next to (P, r - s) (cancel to infinity).  pad random pairs go in front of each, so that the degenerate
    pairs also straddle chunk boundaries."""
    rnd = random.Random(seed)
    ps = point_bytes(cp, group)
    base = cref.gen_points(cp.curve_id, group, 0xED6E + len(seed), 0x77, 8)
    P = [base[i * ps : (i + 1) * ps] for i in range(8)]
    inf = bytes(ps)
    r = cp.r
    s, t, u = (rnd.randrange(1, r) for _ in range(3))
    cases = [
        ([inf, P[0]], [s, t]),
        ([P[0], inf, inf], [s, t, u]),
        ([inf], [s]),
        ([P[0], P[1]], [0, t]),
        ([P[0], P[1], P[2]], [0, 0, 0]),
        ([P[0], P[1]], [s + r, (1 << 256) - 1]),
        ([P[2]], [r]),
        ([P[0], P[0]], [s, s]),
        ([P[0], P[0], P[0], P[0]], [s, s, s, s]),
        ([P[1], P[0], P[0], P[2], P[0]], [t, s, s, u, s]),
        ([P[0], neg_point(cp, group, P[0])], [s, s]),
        ([P[0], P[0]], [s, r - s]),
        ([P[0], neg_point(cp, group, P[0]), P[1]], [s, s, t]),
        ([P[3], P[0], P[0], P[1]], [u, s, r - s, t]),
        ([P[0], P[0], neg_point(cp, group, P[0]), P[0]], [s, s, s, r - s]),
        ([P[4], P[4]], [1, 1]),
        ([P[5], neg_point(cp, group, P[5])], [1, r - 1]),
    ]
    pts, scs, lengths = [], [], []
    for seg_p, seg_s in cases:
        pad_p = [P[6 + (i & 1)] for i in range(pad)]
        pad_s = [rnd.randrange(r) for _ in range(pad)]
        pts += pad_p + seg_p
        scs += pad_s + seg_s
        lengths.append(pad + len(seg_p))
    return b"".join(pts), b"".join(sc(v) for v in scs), lengths


def expected(cp, group: int, pts: bytes, scs: bytes, lengths, mont: bool):
    """cref.msm of every segment (empty: the point at infinity, all zero)"""
    ps = point_bytes(cp, group)
    out, o = [], 0
    for m in lengths:
        out.append(cref.msm(cp.curve_id, group, pts[o * ps : (o + m) * ps], scs[32 * o : 32 * (o + m)], m, mont, 0, 1))
        o += m
    return out


def curve(name: str):
    return R.CURVES[name]
