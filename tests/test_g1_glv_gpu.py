"""The GLV lattice split of BN254 G1 on the GPU: mlhip_scalar_mul* with MLHIP_GROUP_SUBGROUP and mlhip_msm_batch* with
MLHIP_CURVE_SUBGROUP_POINTS on BN254 G1 (mathlib_amd/csrc/msm_scalar_mul_endo.h: g1_glv_split; msm_batch_endo.h).  The flagged
call byte-equal to the plain call on the same buffers and to the oracle -- one lane, a wave less one, a whole wave, a second
wave, whole waves plus a remainder; one base and one point per scalar; both scalar forms; the scalars on the boundaries of
the split; infinities; segments of every length around every chunk length; the degenerate pairs.  The point T = (1, 3), on
y^2 = x^3 + 8 and not on the curve, shows which route ran: with s = lambda the split gives (beta, 3), the value
tests/hostmath_glv gives, where the plain kernels give [lambda]T.  T is ordinary data: no address depends on it."""
import ctypes
import functools
import random

import pytest

from g1_glv_cases import CHUNKS, CP, LAM, T, beta, glv_edge_segments, harness, host_batch, host_mul, scalar_rows
from msm_batch_cases import edge_segments, expected, random_segments
from oracle import pyref as R
from point_sum_cases import distinct_points

pytestmark = pytest.mark.gpu

ENV = ("MLHIP_SCALAR_MUL_ENDO", "MLHIP_FIXED_BASE_MIN", "MLHIP_FB_WINDOW", "MLHIP_FB_CACHE", "MLHIP_SCALAR_MUL_ONE_LANE",
       "MLHIP_MSM_BATCH_ENDO", "MLHIP_MSM_BATCH_CHUNK", "MLHIP_MSM_BATCH_BUCKET_MIN", "MLHIP_MSM_BATCH_BUCKET_SLICE")
CID = 0
PSZ = 64
# 0, 1, 2, 3, P, P + 1 for every compiled P, 17 and 64
LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 17, 64)


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(autouse=True)
def default_routes(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def delay(lib, mlhip):
    """the delay of tests/stream_order_cases.py, calibrated once"""
    import stream_order_cases as S

    d = S.Delay(lib, mlhip)
    assert 50.0 <= d.ms <= 2000.0, (d.repeat, d.ms)
    return d


def at(raw, i):
    return raw[i * PSZ : (i + 1) * PSZ]


def mul(lib, mlhip, flagged, pts, stride, scs, mont, n):
    out = ctypes.create_string_buffer(PSZ * n)
    if flagged:
        mlhip.check(mlhip.scalar_mul_subgroup(lib, CID, 1, pts, stride, scs, mont, n, out))
    else:
        mlhip.check(lib.mlhip_scalar_mul(CID, 1, pts, stride, scs, mont, n, out))
    return out.raw


def batch(lib, mlhip, flagged, pts, scs, mont, lengths):
    k = len(lengths)
    out = ctypes.create_string_buffer(k * PSZ)
    offsets = mlhip.batch_offsets(lengths)
    if flagged:
        mlhip.check(mlhip.msm_batch_subgroup(lib, CID, 1, pts, scs, 1 if mont else 0, offsets, k, out))
    else:
        mlhip.check(lib.mlhip_msm_batch(CID, 1, pts, scs, 1 if mont else 0, offsets, k, out))
    return [at(out.raw, i) for i in range(k)]


@functools.lru_cache(maxsize=None)
def oracle_product(index, k):
    """[k] distinct_points[index] (None: infinity) by oracle/pyref.py, computed once"""
    return R.g1_to_mont_bytes(CP, R.g1_mul(CP, distinct_points("BN254", 1, 300)[index], k))


# ---- mlhip_scalar_mul ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("stride", [1, 0])
def test_flagged_mul_equals_plain_mul_and_oracle(lib, mlhip, stride):
    base = distinct_points("BN254", 1, 300)
    for n in (1, 63, 64, 65, 200):
        pts = list(range(n)) if stride else [0]  # indices into base; None: infinity
        if stride and n >= 3:
            for i in (0, n // 2, n - 1):
                pts[i] = None
        raw = b"".join(R.g1_to_mont_bytes(CP, None if i is None else base[i]) for i in pts)
        for mont in (0, 1):
            rows = scalar_rows(mont)
            assert len(rows) < 200  # n = 200 meets every boundary scalar
            scs = b"".join(rows[(i + n) % len(rows)][0] for i in range(n))
            got = mul(lib, mlhip, True, raw, stride, scs, mont, n)
            plain = mul(lib, mlhip, False, raw, stride, scs, mont, n)
            assert got == plain, (n, stride, mont, [i for i in range(n) if at(got, i) != at(plain, i)][:8])
            for i in (range(n) if n == 200 else sorted({0, min(n // 2 + 1, n - 1), n - 1})):
                p = pts[i if stride else 0]
                want = bytes(PSZ) if p is None else oracle_product(p, rows[(i + n) % len(rows)][1])
                assert at(got, i) == want, (n, stride, mont, i)


def test_off_curve_point_shows_the_route_of_mul(lib, mlhip, monkeypatch):
    """T with s = lambda in the middle of 65 products: the flagged call differs from the plain call in that product only and
    gives the host replay's (beta, 3); the plain value again with MLHIP_SCALAR_MUL_ENDO=0, and on the table path (one base,
    4096 scalars), where the flag changes nothing"""
    n, mid = 65, 32
    base = distinct_points("BN254", 1, 300)
    rows = scalar_rows(0)
    raw = b"".join(R.g1_to_mont_bytes(CP, T if i == mid else base[i]) for i in range(n))
    scs = b"".join(LAM.to_bytes(32, "little") if i == mid else rows[i % len(rows)][0] for i in range(n))
    got = mul(lib, mlhip, True, raw, 1, scs, 0, n)
    plain = mul(lib, mlhip, False, raw, 1, scs, 0, n)
    assert [i for i in range(n) if at(got, i) != at(plain, i)] == [mid]
    assert at(got, mid) == host_mul(harness(), T, LAM.to_bytes(32, "little"), 0) == R.g1_to_mont_bytes(CP, (beta(), 3))
    assert at(plain, mid) == R.g1_to_mont_bytes(CP, R.g1_mul(CP, T, LAM))
    monkeypatch.setenv("MLHIP_SCALAR_MUL_ENDO", "0")
    assert mul(lib, mlhip, True, raw, 1, scs, 0, n) == plain
    monkeypatch.delenv("MLHIP_SCALAR_MUL_ENDO")
    # one base: the split kernel below the fixed-base threshold, the table from it on
    one = R.g1_to_mont_bytes(CP, T)
    for n, table in ((300, False), (4096, True)):
        scs = b"".join(LAM.to_bytes(32, "little") if i == n // 2 else rows[i % len(rows)][0] for i in range(n))
        got = mul(lib, mlhip, True, one, 0, scs, 0, n)
        plain = mul(lib, mlhip, False, one, 0, scs, 0, n)
        if table:
            assert got == plain
        else:
            assert at(got, n // 2) == R.g1_to_mont_bytes(CP, (beta(), 3)) != at(plain, n // 2)


# ---- mlhip_msm_batch -----------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def mixed():
    """70 segments of the lengths above in seeded random order, every length at least four times: at every P more than 64
    chunks (a second wave of lanes); and cref.msm of every segment in both scalar forms"""
    rnd = random.Random("g1-glv-gpu")
    lengths = list(LENGTHS) * 4 + [rnd.choice(LENGTHS) for _ in range(30)]
    rnd.shuffle(lengths)
    assert len(lengths) == 70 and sum(-(-m // 8) for m in lengths) > 64
    pts, scs, lengths = random_segments(CP, 1, lengths, "g1-glv-gpu")
    return pts, scs, lengths, {mont: expected(CP, 1, pts, scs, lengths, mont) for mont in (False, True)}


def set_chunk(monkeypatch, P):
    if P is None:
        monkeypatch.delenv("MLHIP_MSM_BATCH_CHUNK", raising=False)
    else:
        monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", str(P))


def test_flagged_batch_equals_plain_batch_and_cref(lib, mlhip, monkeypatch):
    pts, scs, lengths, exp = mixed()
    for P in (None,) + CHUNKS:
        set_chunk(monkeypatch, P)
        for mont in (False, True):
            got = batch(lib, mlhip, True, pts, scs, mont, lengths)
            bad = [i for i in range(len(lengths)) if got[i] != exp[mont][i]]
            assert not bad, (P, mont, bad[:10], [lengths[i] for i in bad[:10]])
            assert batch(lib, mlhip, False, pts, scs, mont, lengths) == exp[mont], (P, mont)


def test_degenerate_pairs_inside_one_chunk(lib, mlhip, monkeypatch):
    for make in (lambda seed, pad: edge_segments(CP, 1, seed, pad), glv_edge_segments):
        for pad in (0, 1, 3):
            pts, scs, lengths = make("g1-glv-gpu-edge", pad)
            for mont in (False, True):
                exp = expected(CP, 1, pts, scs, lengths, mont)
                for P in (None,) + CHUNKS:
                    set_chunk(monkeypatch, P)
                    got = batch(lib, mlhip, True, pts, scs, mont, lengths)
                    assert got == exp, (pad, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])
                    if P is None:
                        assert batch(lib, mlhip, False, pts, scs, mont, lengths) == exp


def with_witness(lengths, seg, seed):
    """random segments; the middle pair of segment `seg` replaced by (T, lambda)"""
    pts, scs, lengths = random_segments(CP, 1, lengths, seed)
    i = sum(lengths[:seg]) + lengths[seg] // 2
    pts = pts[: i * PSZ] + R.g1_to_mont_bytes(CP, T) + pts[(i + 1) * PSZ :]
    scs = scs[: 32 * i] + LAM.to_bytes(32, "little") + scs[32 * (i + 1) :]
    return pts, scs, lengths


def test_off_curve_point_shows_the_route_of_the_chunks(lib, mlhip, monkeypatch):
    """nine segments, T in the middle one: the flagged call differs from the plain call in that segment only and gives what
    the split chunk body gives on the CPU; MLHIP_MSM_BATCH_ENDO=0 runs the plain chunk kernel"""
    pts, scs, lengths = with_witness([2, 5, 0, 1, 3, 4, 9, 2, 6], 4, "g1-glv-gpu-route")
    glv = harness()
    for P in (None,) + CHUNKS:
        set_chunk(monkeypatch, P)
        plain = batch(lib, mlhip, False, pts, scs, False, lengths)
        got = batch(lib, mlhip, True, pts, scs, False, lengths)
        assert [i for i in range(9) if got[i] != plain[i]] == [4], P
        rc, host = host_batch(glv, P or 4, pts, scs, lengths, False)
        assert rc == 0 and got == host, P
        monkeypatch.setenv("MLHIP_MSM_BATCH_ENDO", "0")
        assert batch(lib, mlhip, True, pts, scs, False, lengths) == plain
        monkeypatch.delenv("MLHIP_MSM_BATCH_ENDO")


def test_long_segment_still_takes_the_bucket_route(lib, mlhip, monkeypatch):
    """one segment of 600 pairs among short ones, T inside it: the bucket route does not look at the flag, so the flagged call
    equals the plain one in every segment -- and stops doing so in that segment alone once MLHIP_MSM_BATCH_BUCKET_MIN=0 sends
    the long segment to the chunks"""
    pts, scs, lengths = with_witness([3, 0, 17, 600, 1, 5, 64], 3, "g1-glv-gpu-bucket")
    assert batch(lib, mlhip, True, pts, scs, False, lengths) == batch(lib, mlhip, False, pts, scs, False, lengths)
    monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_MIN", "0")
    plain = batch(lib, mlhip, False, pts, scs, False, lengths)
    chunks = batch(lib, mlhip, True, pts, scs, False, lengths)
    assert [i for i in range(len(lengths)) if chunks[i] != plain[i]] == [3]


# ---- the _device forms and the Python mirrors --------------------------------------------------------------------------


def test_device_form_of_mul_on_a_busy_stream(lib, mlhip, delay):
    import torch

    import stream_order_cases as S

    class ScalarMulSubgroup(S.ScalarMul):
        def call(self, lib, mlhip, ins, outs, host, stream):
            mlhip.check(mlhip.scalar_mul_subgroup_device(lib, self.cid, self.group, ins[0], self.stride, ins[1], 0, self.n, outs[0], stream))
            return []

        def host_form(self, lib, mlhip, ins, host):
            out = ctypes.create_string_buffer(self.psz * self.n)
            mlhip.check(mlhip.scalar_mul_subgroup(lib, self.cid, self.group, ins[0], self.stride, ins[1], 0, self.n, out))
            return [out.raw]

    lines = []
    outcome = S.run_scenario(lib, mlhip, ScalarMulSubgroup(CID, 1, 1, 300), torch.cuda.Stream(), delay, lines.append,
                             "scalar-mul-subgroup-g1-glv")
    assert outcome.busy and lines


def test_device_form_of_batch_on_a_busy_stream(lib, mlhip, delay):
    import torch

    import stream_order_cases as S

    class MsmBatchSubgroup(S.MsmBatch):
        def call(self, lib, mlhip, ins, outs, host, stream):
            mlhip.check(mlhip.msm_batch_subgroup_device(lib, self.cid, self.group, ins[0], ins[1], 0, host["offsets"], self.k, outs[0], stream))
            return []

        def host_form(self, lib, mlhip, ins, host):
            out = ctypes.create_string_buffer(self.psz * self.k)
            mlhip.check(mlhip.msm_batch_subgroup(lib, self.cid, self.group, ins[0], ins[1], 0, host["offsets"], self.k, out))
            return [out.raw]

    lines = []
    outcome = S.run_scenario(lib, mlhip, MsmBatchSubgroup(CID, 1), torch.cuda.Stream(), delay, lines.append,
                             "msm-batch-subgroup-g1-glv")
    assert outcome.busy and lines


def test_python_mirrors(lib, mlhip):
    """MulBatchSubgroup / MultiScalarMulBatchSubgroup of mathlib_amd/driver.py equal the plain mirrors on BN254 G1, and
    msm_batch(subgroup=True) of mathlib_amd/_lib.py reaches the split: T alone in a segment comes back as (beta, 3)"""
    from mathlib_amd.driver import Curve

    c = Curve(CID)
    rng = random.Random("g1-glv-mirror")
    g1 = c.GenG1()
    zs = [c.NewZrFromInt(v) for v in (-1, LAM, LAM + 1, CP.r - LAM, 1 << 127, 0)] + [c.GroupOrder] + [c.NewRandomZr(rng.randrange) for _ in range(5)]
    pts = [g1.Mul(c.NewZrFromInt(rng.randrange(1, CP.r))) for _ in range(len(zs) - 1)] + [g1]
    fast = c.MulBatchSubgroup(pts, zs)
    assert [p.raw for p in fast] == [p.raw for p in c.MulBatch(pts, zs)]
    assert fast[0].raw == pts[0].Mul(zs[0]).raw and fast[1].raw == pts[1].Mul(zs[1]).raw and fast[5].IsInfinity() and fast[6].IsInfinity()
    a_lists, b_lists = [pts[:3], [], pts[3:4], pts[4:12], pts[5:7]], [zs[:3], [], zs[3:4], zs[4:12], zs[5:7]]
    got = c.MultiScalarMulBatchSubgroup(a_lists, b_lists)
    assert [p.raw for p in got] == [p.raw for p in c.MultiScalarMulBatch(a_lists, b_lists)]
    assert got[0].Equals(c.MultiScalarMul(a_lists[0], b_lists[0])) and got[1].IsInfinity()
    raw = mlhip.msm_batch(CID, 1, R.g1_to_mont_bytes(CP, T), LAM.to_bytes(32, "little"), False, [1], subgroup=True)
    assert [bytes(b) for b in raw] == [R.g1_to_mont_bytes(CP, (beta(), 3))]
