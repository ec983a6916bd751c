"""Inputs and expected outputs of the segmented point-sum tests (tests/test_sum_batch_host.py, tests/test_sum_batch_gpu.py,
tests/test_sum_batch_stream_order_gpu.py): one batch per curve and group whose segments are the compositions of
tests/point_sum_cases.py -- a repeated point (doubling), P, -P pairs, an all-infinity list, a list that sums to infinity and
a point of the curve outside the prime-order subgroup -- with oracle.pyref's affine additions as the expected bytes.

The segment lengths are chosen for a slice length S forced to 4 (MLHIP_SUM_BATCH_SLICE=4): empty segments at the front and in
the middle, 1 .. 5 and 9 points (one slice, a full slice, one more than a full slice, three slices of 3), 128 = 32 slices
(the longest segment whose slice sums still fit the last pass), 129 = 32 * 4 + 1 (33 slices: the smallest segment that needs
a middle sum pass) and 33.  The same list runs at the default S (4 for a call this small).  314 points in all."""
import functools

from point_sum_cases import composition, curve, expected, ops, pack, point_bytes

LENGTHS = [0, 1, 2, 3, 4, 5, 9, 0, 128, 129, 33]
KINDS = [None, "repeated", "pairs", "sums_to_infinity", "outside_subgroup", "all_infinity", "pairs", None, "repeated",
         "outside_subgroup", "sums_to_infinity"]
TOTAL = sum(LENGTHS)
assert TOTAL < 400 and len(KINDS) == len(LENGTHS)


def offsets_of(lengths):
    out = [0]
    for m in lengths:
        out.append(out[-1] + m)
    return out


@functools.lru_cache(maxsize=None)
def segments(name: str, group: int):
    """the point lists (None = infinity) of the batch; BN254's G1 has no point outside the subgroup: its two such segments
    are lists with infinities at the first, middle and last position instead"""
    out = []
    for m, kind in zip(LENGTHS, KINDS):
        if m == 0:
            out.append([])
            continue
        pts = composition(name, group, kind, m)
        if pts is None:
            assert (name, group, kind) == ("BN254", 1, "outside_subgroup")
            pts = composition(name, group, "infinities", m)
        assert len(pts) == m
        out.append(pts)
    return tuple(tuple(s) for s in out)


@functools.lru_cache(maxsize=None)
def batch(name: str, group: int):
    """(all points in the C-ABI layout, the expected affine sum of every segment), computed once per session"""
    cp = curve(name)
    segs = segments(name, group)
    return b"".join(pack(cp, group, s) for s in segs), tuple(expected(cp, group, s) for s in segs)


@functools.lru_cache(maxsize=None)
def indexed_batch(name: str, group: int, n_bases: int = 40):
    """(the bases in the C-ABI layout, index lists, expected sums with the lists, lengths, expected sums of the first lengths[i]
    bases): n_bases bases taken from the batch's 129-point segment (on BLS12 curves one of them lies outside the subgroup),
    index lists with repeats, with one base used in two segments, an empty one and one longer than four slices of 4"""
    cp = curve(name)
    long = segments(name, group)[9]
    bases = list(long[len(long) // 2 - n_bases // 2 : len(long) // 2 - n_bases // 2 + n_bases])
    bases[3] = None  # an infinity among the bases
    lists = [[5, 5, 5, 7], [], [7, 0, 39, 3], [n_bases // 2], [(i * 7) % n_bases for i in range(37)], [39, 38, 37]]
    lengths = [0, 1, 4, 5, 17, n_bases]
    exp_lists = tuple(expected(cp, group, [bases[i] for i in ix]) for ix in lists)
    exp_lengths = tuple(expected(cp, group, bases[:m]) for m in lengths)
    return pack(cp, group, bases), lists, exp_lists, lengths, exp_lengths


__all__ = ["LENGTHS", "KINDS", "TOTAL", "offsets_of", "segments", "batch", "indexed_batch", "curve", "ops", "point_bytes"]
