"""Inputs and expected outputs of the batched MSM over resident bases (tests/test_bases_batch_host.py,
tests/test_bases_batch_gpu.py): segments as lists of (base index, scalar) over a small set of bases, and the degenerate
segments of tests/msm_batch_cases.py rewritten as indices into the distinct points they use, with cref.msm of every segment
over the gathered points as the expected bytes."""
import random

from msm_batch_cases import edge_segments, expected, point_bytes, sc
from oracle import cref


def gen_bases(cp, group: int, n: int, seed: int) -> bytes:
    return cref.gen_points(cp.curve_id, group, 0xBA5E + seed, 0x5EED + n, n)


def gather(cp, group: int, bases: bytes, index) -> bytes:
    ps = point_bytes(cp, group)
    return b"".join(bases[i * ps : (i + 1) * ps] for i in index)


def random_indexed(cp, n: int, lengths, seed: str):
    """segments of the given lengths: random base indices below n (repeats allowed), uniform 256-bit scalars"""
    rnd = random.Random(seed)
    total = sum(lengths)
    index = [rnd.randrange(n) for _ in range(total)]
    scs = b"".join(sc(rnd.getrandbits(256)) for _ in range(total))
    return index, scs


def positional_index(lengths):
    """the indices a call without an index list reads: pair j of a segment takes base j"""
    return [j for m in lengths for j in range(m)]


def edge_indexed(cp, group: int, seed: str, pad: int = 0):
    """msm_batch_cases.edge_segments over a handle: (bases, index, scalars, lengths) with the distinct points as bases (the
    point at infinity and -P among them) and every pair naming its point by index"""
    pts, scs, lengths = edge_segments(cp, group, seed, pad)
    ps = point_bytes(cp, group)
    uniq, index = [], []
    for i in range(len(pts) // ps):
        p = pts[i * ps : (i + 1) * ps]
        if p not in uniq:
            uniq.append(p)
        index.append(uniq.index(p))
    return b"".join(uniq), index, scs, lengths


def expected_indexed(cp, group: int, bases: bytes, index, scs: bytes, lengths, mont: bool):
    return expected(cp, group, gather(cp, group, bases, index), scs, lengths, mont)
