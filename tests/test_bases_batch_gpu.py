"""The batched MSM over resident bases on the GPU (mlhip_bases_msm_batch / _device / mlhip_bases_batch_tabled,
mathlib_amd/csrc/msm_bases_batch.h): byte equality with cref.msm for every segment -- every curve, G1 and G2, Montgomery
and plain non-canonical scalars, with and without an index list, mixed segment lengths 0 .. n in random order and segments
longer than the chunk length; bases at infinity, repeated indices, (B, s) beside (B, r - s); the table path against
MLHIP_BASES_BATCH_MAX_MB=0 (the table-free path) and mlhip_msm_batch over the gathered points; tables that grow; the device
form on a non-default stream, two host threads on one handle, argument checks, and the Python mirror."""
import ctypes
import random
import threading

import pytest

from bases_batch_cases import edge_indexed, expected_indexed, gather, gen_bases, positional_index, random_indexed
from msm_batch_cases import CURVES, curve, point_bytes

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


class Handle:
    def __init__(self, lib, cp, group, bases: bytes):
        self.lib, self.cp, self.group = lib, cp, group
        self.ps = point_bytes(cp, group)
        self.n = len(bases) // self.ps
        self.h = ctypes.c_void_p()
        assert lib.mlhip_bases_create(cp.curve_id, group, bases, self.n, 0, ctypes.byref(self.h)) == 0

    def batch(self, mlhip, scs, mont, lengths, index=None):
        lists = None
        if index is not None:
            lists, o = [], 0
            for m in lengths:
                lists.append(index[o : o + m])
                o += m
        return mlhip.bases_msm_batch(self.lib, self.h, self.ps, scs, mont, lengths, lists)

    def tabled(self, mlhip):
        return mlhip.bases_batch_tabled(self.lib, self.h)

    def close(self):
        if self.h:
            self.lib.mlhip_bases_destroy(self.h)
            self.h = ctypes.c_void_p()


def mixed_lengths(seed: str, n: int):
    rnd = random.Random(seed)
    lengths = list(range(n + 1)) + [rnd.randrange(n + 1) for _ in range(60)]
    rnd.shuffle(lengths)
    return lengths


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_mixed_segments_match_cref(lib, mlhip, name, group):
    cp = curve(name)
    n = 24  # longer than every chunk length: segments of 17 .. 24 pairs span several chunks
    bases = gen_bases(cp, group, n, 10)
    h = Handle(lib, cp, group, bases)
    try:
        lengths = mixed_lengths("gpu-mixed/%s/%d" % (name, group), n)
        index, scs = random_indexed(cp, n, lengths, "gpu-mixed/%s/%d" % (name, group))
        pos = positional_index(lengths)
        for mont in (False, True):
            for idx in (index, None):
                got = h.batch(mlhip, scs, mont, lengths, idx)
                exp = expected_indexed(cp, group, bases, pos if idx is None else idx, scs, lengths, mont)
                bad = [i for i in range(len(exp)) if got[i] != exp[i]]
                assert not bad, (name, group, mont, idx is None, bad[:10], [lengths[i] for i in bad[:10]])
        assert h.tabled(mlhip) == n
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_degenerate_segments(lib, mlhip, name, group):
    """bases at infinity, zero scalars, scalars >= r, repeated indices, (B, s) beside (-B, s) and (B, r - s)"""
    cp = curve(name)
    for pad in (0, 3):
        bases, index, scs, lengths = edge_indexed(cp, group, "gpu-edge/%s/%d" % (name, group), pad)
        assert bytes(point_bytes(cp, group)) in [bases[i : i + point_bytes(cp, group)] for i in range(0, len(bases), point_bytes(cp, group))]
        h = Handle(lib, cp, group, bases)
        try:
            for mont in (False, True):
                exp = expected_indexed(cp, group, bases, index, scs, lengths, mont)
                got = h.batch(mlhip, scs, mont, lengths, index)
                assert got == exp, (name, group, pad, mont, [i for i in range(len(exp)) if got[i] != exp[i]])
        finally:
            h.close()


@pytest.mark.parametrize("group", [1, 2])
def test_same_base_repeated_and_cancelling(lib, mlhip, group):
    cp = curve("BLS12-381")
    r = cp.r
    bases = gen_bases(cp, group, 4, 11)
    vals = [[1, 1], [1, 1, 1, 1], [5, r - 5], [7, r - 7, 7], [r - 1, 1, 2], [(1 << 256) - 1, 1]]
    lengths = [len(v) for v in vals]
    scs = b"".join(x.to_bytes(32, "little") for v in vals for x in v)
    index = [2] * sum(lengths)
    exp = expected_indexed(cp, group, bases, index, scs, lengths, False)
    assert exp[2] == bytes(point_bytes(cp, group))
    h = Handle(lib, cp, group, bases)
    try:
        assert h.batch(mlhip, scs, False, lengths, index) == exp
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_table_path_equals_table_free_and_msm_batch(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    n = 64
    bases = gen_bases(cp, group, n, 12)
    lengths = [random.Random(name).randrange(0, 17) for _ in range(300)]
    index, scs = random_indexed(cp, n, lengths, "gpu-paths/%s/%d" % (name, group))
    ref = mlhip.msm_batch(cp.curve_id, group, gather(cp, group, bases, index), scs, True, lengths)
    h = Handle(lib, cp, group, bases)
    try:
        monkeypatch.setenv("MLHIP_BASES_BATCH_MAX_MB", "0")
        free = h.batch(mlhip, scs, True, lengths, index)
        assert h.tabled(mlhip) == 0  # the table-free path ran and built nothing
        monkeypatch.delenv("MLHIP_BASES_BATCH_MAX_MB")
        tab = h.batch(mlhip, scs, True, lengths, index)
        assert h.tabled(mlhip) == max(index) + 1
        assert tab == free == ref
        # with tables present, a cap they would pass sends the call to the table-free path again, tables kept
        monkeypatch.setenv("MLHIP_BASES_BATCH_MAX_MB", "0")
        assert h.batch(mlhip, scs, True, lengths, index) == ref
        assert h.tabled(mlhip) == max(index) + 1
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 2])
def test_widths_and_chunk_lengths(lib, mlhip, monkeypatch, group):
    """every allowed chunk length and the extreme widths (a new width rebuilds the tables) give the same bytes"""
    cp = curve("BN254")
    n = 20
    bases = gen_bases(cp, group, n, 13)
    lengths = [random.Random(7).randrange(0, 21) for _ in range(80)]
    index, scs = random_indexed(cp, n, lengths, "gpu-wp/%d" % group)
    exp = expected_indexed(cp, group, bases, index, scs, lengths, False)
    h = Handle(lib, cp, group, bases)
    try:
        for w, P in ((4, 1), (12, 16), (5, 2), (8, 4), (6, 8), (8, 16)):
            monkeypatch.setenv("MLHIP_BASES_BATCH_WINDOW", str(w))
            monkeypatch.setenv("MLHIP_BASES_BATCH_CHUNK", str(P))
            assert h.batch(mlhip, scs, False, lengths, index) == exp, (w, P)
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 2])
def test_tables_grow(lib, mlhip, monkeypatch, group):
    cp = curve("BLS12-381")
    n = 256
    monkeypatch.setenv("MLHIP_BASES_BATCH_WINDOW", "8")  # 201 G2 bases at the default width would pass the default cap
    bases = gen_bases(cp, group, n, 14)
    h = Handle(lib, cp, group, bases)
    try:
        assert h.tabled(mlhip) == 0  # nothing until a batch call
        lengths = [3, 5, 0, 8, 2]
        index, scs = random_indexed(cp, 8, lengths, "gpu-grow-a/%d" % group)
        index[0] = 7
        assert h.batch(mlhip, scs, False, lengths, index) == expected_indexed(cp, group, bases, index, scs, lengths, False)
        assert h.tabled(mlhip) == 8
        lengths = [4, 16, 1, 9]
        index, scs = random_indexed(cp, 201, lengths, "gpu-grow-b/%d" % group)
        index[-1] = 200
        assert h.batch(mlhip, scs, True, lengths, index) == expected_indexed(cp, group, bases, index, scs, lengths, True)
        assert h.tabled(mlhip) == 201
        # the first bases' rows were carried over: a call on them alone is still right
        lengths = [6]
        index, scs = random_indexed(cp, 8, lengths, "gpu-grow-c/%d" % group)
        assert h.batch(mlhip, scs, False, lengths, index) == expected_indexed(cp, group, bases, index, scs, lengths, False)
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 2])
def test_device_form_on_a_non_default_stream(lib, mlhip, group):
    import torch

    cp = curve("BN254")
    n = 16
    bases = gen_bases(cp, group, n, 15)
    lengths = mixed_lengths("gpu-stream/%d" % group, n)
    index, scs = random_indexed(cp, n, lengths, "gpu-stream/%d" % group)
    ps = point_bytes(cp, group)
    K = len(lengths)
    h = Handle(lib, cp, group, bases)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ds = torch.frombuffer(bytearray(scs), dtype=torch.uint8).cuda()
            out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
            mlhip.check(lib.mlhip_bases_msm_batch_device(h.h, ds.data_ptr(), 1, mlhip.batch_index([index]), mlhip.batch_offsets(lengths),
                                                         K, s.cuda_stream, out.data_ptr()))
            got = out.cpu().numpy().tobytes()  # on s: ordered after the batch
        s.synchronize()
        assert got == b"".join(expected_indexed(cp, group, bases, index, scs, lengths, True))
    finally:
        h.close()


def test_two_threads_on_one_handle(lib, mlhip):
    cp = curve("BLS12-381")
    n = 40
    bases = gen_bases(cp, 1, n, 16)
    h = Handle(lib, cp, 1, bases)
    jobs = []
    for t in range(2):
        lengths = [random.Random(t).randrange(0, 9) for _ in range(200)]
        # thread 1 reads further than thread 0: whichever comes second may grow the tables under the other's feet
        index, scs = random_indexed(cp, 10 if t == 0 else n, lengths, "gpu-threads/%d" % t)
        jobs.append((lengths, index, scs, expected_indexed(cp, 1, bases, index, scs, lengths, False)))
    errors = []

    def work(j):
        lengths, index, scs, exp = jobs[j]
        try:
            for _ in range(4):
                assert h.batch(mlhip, scs, False, lengths, index) == exp
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((j, e))

    try:
        th = [threading.Thread(target=work, args=(j,)) for j in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
    finally:
        h.close()


def test_argument_checks(lib, mlhip):
    cp = curve("BLS12-381")
    n = 4
    bases = gen_bases(cp, 1, n, 17)
    h = Handle(lib, cp, 1, bases)
    out = ctypes.create_string_buffer(2 * 96)
    scs = bytes(32 * 8)

    def offs(*v):
        return (ctypes.c_uint64 * len(v))(*v)

    def idx(*v):
        return (ctypes.c_uint32 * len(v))(*v)

    try:
        # K = 0: nothing to do, nothing touched
        assert lib.mlhip_bases_msm_batch(h.h, None, 0, None, None, 0, None) == 0
        assert lib.mlhip_bases_msm_batch_device(h.h, None, 0, None, None, 0, None, None) == 0
        assert mlhip.bases_msm_batch(lib, h.h, 96, b"", False, []) == []
        # malformed offsets
        for bad in (offs(0, 3, 2), offs(1, 3, 5), offs(0, 5, 4)):
            assert lib.mlhip_bases_msm_batch(h.h, scs, 0, None, bad, 2, out) == EINVAL
            assert lib.mlhip_bases_msm_batch_device(h.h, scs, 0, None, bad, 2, None, out) == EINVAL
        assert lib.mlhip_bases_msm_batch(h.h, scs, 0, None, None, 2, out) == EINVAL
        # an index >= n, and a segment longer than n without an index list
        assert lib.mlhip_bases_msm_batch(h.h, scs, 0, idx(0, 1, 4), offs(0, 1, 3), 2, out) == EINVAL
        assert lib.mlhip_bases_msm_batch_device(h.h, scs, 0, idx(0, 1, 4), offs(0, 1, 3), 2, None, out) == EINVAL
        assert lib.mlhip_bases_msm_batch(h.h, scs, 0, None, offs(0, 1, 6), 2, out) == EINVAL
        assert lib.mlhip_bases_msm_batch_device(h.h, scs, 0, None, offs(0, 1, 6), 2, None, out) == EINVAL
        # null pointers
        assert lib.mlhip_bases_msm_batch(None, scs, 0, None, offs(0, 1, 3), 2, out) == EINVAL
        assert lib.mlhip_bases_msm_batch(h.h, None, 0, None, offs(0, 1, 3), 2, out) == EINVAL
        assert lib.mlhip_bases_msm_batch(h.h, scs, 0, None, offs(0, 1, 3), 2, None) == EINVAL
        tabled = ctypes.c_size_t(99)
        assert lib.mlhip_bases_batch_tabled(None, ctypes.byref(tabled)) == EINVAL
        assert lib.mlhip_bases_batch_tabled(h.h, None) == EINVAL
        assert h.tabled(mlhip) == 0  # no refused call built anything
        # all segments empty: every output is the point at infinity, no tables
        assert lib.mlhip_bases_msm_batch(h.h, None, 0, None, offs(0, 0, 0), 2, out) == 0
        assert out.raw == bytes(2 * 96) and h.tabled(mlhip) == 0
        # a segment of exactly n pairs, after the refusals
        lengths = [4, 1]
        s2 = b"".join((i + 3).to_bytes(32, "little") for i in range(5))
        got = mlhip.bases_msm_batch(lib, h.h, 96, s2, False, lengths)
        assert got == expected_indexed(cp, 1, bases, positional_index(lengths), s2, lengths, False)
    finally:
        h.close()


@pytest.mark.parametrize("name", CURVES)
def test_python_mirror(lib, name):
    from mathlib_amd.driver import Curve

    cp = curve(name)
    cv = Curve(cp.curve_id)
    rng = random.Random("mirror/" + name)
    g = cv.GenG1()
    pts = [g.Mul(cv.NewZrFromInt(rng.randrange(1, cp.r))) for _ in range(10)]
    zr = [cv.NewRandomZr(rng.randrange) for _ in range(40)]
    b = cv.NewBases(pts)
    try:
        scal = [zr[:3], [], zr[3:13], zr[13:14]]
        got = b.MultiScalarMulBatch(scal)
        for x, s in zip(got, scal):
            assert x.Equals(b.MultiScalarMul(s))
        assert got[1].IsInfinity()
        index = [[9, 0, 9], [], [rng.randrange(10) for _ in range(10)], [4]]
        got = b.MultiScalarMulBatch(scal, index)
        for x, s, ix in zip(got, scal, index):
            assert x.Equals(cv.MultiScalarMul([pts[i] for i in ix], s))
        assert b.BatchTabled() == 10
        with pytest.raises(IndexError):
            b.MultiScalarMulBatch([zr[:11]])
        with pytest.raises(IndexError):
            b.MultiScalarMulBatch([zr[:2]], [[0, 10]])
        with pytest.raises(ValueError):
            b.MultiScalarMulBatch([zr[:2]], [[0]])
        assert b.MultiScalarMulBatch([]) == []
    finally:
        b.Close()
