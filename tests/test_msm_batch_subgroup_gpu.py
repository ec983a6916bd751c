"""mlhip_msm_batch / mlhip_msm_batch_device with MLHIP_CURVE_SUBGROUP_POINTS on the GPU: the endomorphism-split Straus chunks
of mathlib_amd/csrc/msm_batch_endo.h.  Every curve and both groups: the flagged call byte-equal to the plain call on the same
buffers and to cref.msm of every segment -- segments of every length around every compiled chunk length in random order
(a second wave of lanes and of lane pairs), uniform 256-bit and Montgomery scalars, every compiled P and the default, the
degenerate pairs of tests/msm_batch_cases.py and the ones the endomorphism adds.  A point OUTSIDE the subgroup shows which
route ran: the split chunk gives the value tests/hostmath_batch_endo gives for it, the plain chunk and the bucket route the
true sum."""
import ctypes
import functools
import random

import pytest

from msm_batch_cases import edge_segments, expected, point_bytes, random_segments
from msm_batch_subgroup_cases import (CHUNKS, CURVES, SPLIT, endo_edge_segments, endo_scalar, harness, host_batch, mul,
                                      to_bytes)
from point_sum_cases import distinct_points, outside_subgroup_point

pytestmark = pytest.mark.gpu

ENV = ("MLHIP_MSM_BATCH_ENDO", "MLHIP_MSM_BATCH_CHUNK", "MLHIP_MSM_BATCH_BUCKET_MIN", "MLHIP_MSM_BATCH_BUCKET_SLICE")
ALL = [(name, group) for name in CURVES for group in (1, 2)]
# 0, 1, 2, 3, P, P + 1 for every compiled P, 17 and 64
LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 17, 64)


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the batched MSM has no CPU fallback"
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


def curve(name):
    from oracle import pyref as R

    return R.CURVES[name]


def batch(lib, mlhip, cp, group, flagged, pts, scs, mont, lengths):
    ps = point_bytes(cp, group)
    k = len(lengths)
    out = ctypes.create_string_buffer(k * ps)
    offsets = mlhip.batch_offsets(lengths)
    if flagged:
        mlhip.check(mlhip.msm_batch_subgroup(lib, cp.curve_id, group, pts, scs, 1 if mont else 0, offsets, k, out))
    else:
        mlhip.check(lib.mlhip_msm_batch(cp.curve_id, group, pts, scs, 1 if mont else 0, offsets, k, out))
    return [out.raw[i * ps : (i + 1) * ps] for i in range(k)]


@functools.lru_cache(maxsize=None)
def mixed(name, group):
    """70 segments of the lengths above in seeded random order, every length at least four times: at every compiled P more
    than 64 chunks (a second wave of G1 lanes, a third of G2 lane pairs); and cref.msm of every segment in both scalar forms"""
    cp = curve(name)
    rnd = random.Random("subgroup-gpu/%s/%d" % (name, group))
    lengths = list(LENGTHS) * 4 + [rnd.choice(LENGTHS) for _ in range(30)]
    rnd.shuffle(lengths)
    assert len(lengths) == 70 and sum(-(-m // 8) for m in lengths) > 64
    pts, scs, lengths = random_segments(cp, group, lengths, "subgroup-gpu/%s/%d" % (name, group))
    return pts, scs, lengths, {mont: expected(cp, group, pts, scs, lengths, mont) for mont in (False, True)}


@pytest.mark.parametrize("name,group", ALL)
def test_flagged_call_equals_plain_call_and_cref(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    pts, scs, lengths, exp = mixed(name, group)
    for P in (None,) + CHUNKS[group]:
        if P is not None:
            monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", str(P))
        for mont in (False, True):
            got = batch(lib, mlhip, cp, group, True, pts, scs, mont, lengths)
            plain = batch(lib, mlhip, cp, group, False, pts, scs, mont, lengths)
            bad = [i for i in range(len(lengths)) if got[i] != exp[mont][i]]
            assert not bad, (name, group, P, mont, bad[:10], [lengths[i] for i in bad[:10]])
            assert plain == exp[mont], (name, group, P, mont)


@pytest.mark.parametrize("name,group", ALL)
def test_degenerate_pairs_inside_one_chunk(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    makers = (edge_segments, endo_edge_segments) if (name, group) in SPLIT else (edge_segments,)
    for make in makers:
        for pad in (0, 1, 3):
            pts, scs, lengths = make(cp, group, "subgroup-gpu-edge/%s/%d" % (name, group), pad)
            for mont in (False, True):
                exp = expected(cp, group, pts, scs, lengths, mont)
                for P in (None,) + CHUNKS[group]:
                    if P is None:
                        monkeypatch.delenv("MLHIP_MSM_BATCH_CHUNK", raising=False)
                    else:
                        monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", str(P))
                    got = batch(lib, mlhip, cp, group, True, pts, scs, mont, lengths)
                    assert got == exp, (make.__name__, name, group, pad, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])
                    if P is None:
                        assert batch(lib, mlhip, cp, group, False, pts, scs, mont, lengths) == exp


def with_outsider(name, group, lengths, seg, seed):
    """random segments of the subgroup; the middle pair of segment `seg` replaced by a point outside the subgroup (where the
    group has one) with the scalar whose split is a single digit 1 on the endomorphism's image"""
    cp = curve(name)
    pts, scs, lengths = random_segments(cp, group, lengths, seed)
    T = outside_subgroup_point(name, group)
    if T is not None:
        ps = point_bytes(cp, group)
        at = sum(lengths[:seg]) + lengths[seg] // 2
        pts = pts[: at * ps] + to_bytes(cp, group, T) + pts[(at + 1) * ps :]
        scs = scs[: 32 * at] + endo_scalar(cp, group).to_bytes(32, "little") + scs[32 * (at + 1) :]
    return pts, scs, lengths


@pytest.mark.parametrize("name,group", ALL)
def test_long_segment_still_takes_the_bucket_route(lib, mlhip, monkeypatch, name, group):
    """one segment of 600 (G1) / 300 (G2) pairs among short ones, a point outside the subgroup inside it: the bucket route is
    exact for every point of the curve, so the flagged call equals the plain one in every segment -- and stops doing so in
    that segment alone once MLHIP_MSM_BATCH_BUCKET_MIN=0 sends the long segment to the split chunks"""
    cp = curve(name)
    long = 600 if group == 1 else 300
    lengths = [3, 0, 17, long, 1, 5, 64]
    pts, scs, lengths = with_outsider(name, group, lengths, 3, "subgroup-gpu-bucket/%s/%d" % (name, group))
    plain = batch(lib, mlhip, cp, group, False, pts, scs, False, lengths)
    assert batch(lib, mlhip, cp, group, True, pts, scs, False, lengths) == plain
    monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_MIN", "0")
    assert batch(lib, mlhip, cp, group, False, pts, scs, False, lengths) == plain
    chunks = batch(lib, mlhip, cp, group, True, pts, scs, False, lengths)
    assert [i for i in range(len(lengths)) if chunks[i] != plain[i]] == ([3] if (name, group) in SPLIT else [])


@pytest.mark.parametrize("name,group", ALL)
def test_point_outside_the_subgroup_shows_the_route(lib, mlhip, monkeypatch, name, group):
    """nine segments, a point outside the subgroup in the middle one: the flagged call differs from the plain call in that
    segment only and gives what the split chunk body gives on the CPU; MLHIP_MSM_BATCH_ENDO=0, BN254 G1 and G2 at P = 8 run the
    plain chunk kernel"""
    cp = curve(name)
    lengths = [2, 5, 0, 1, 3, 4, 9, 2, 6]
    pts, scs, lengths = with_outsider(name, group, lengths, 4, "subgroup-gpu-route/%s/%d" % (name, group))
    plain = batch(lib, mlhip, cp, group, False, pts, scs, False, lengths)
    assert plain == expected(cp, group, pts, scs, lengths, False)  # (cref.msm is defined for every point of the curve)
    if (name, group) not in SPLIT:
        assert batch(lib, mlhip, cp, group, True, pts, scs, False, lengths) == plain
        monkeypatch.setenv("MLHIP_MSM_BATCH_ENDO", "0")
        assert batch(lib, mlhip, cp, group, True, pts, scs, False, lengths) == plain
        return
    hbe = harness()
    for P in (None,) + CHUNKS[group]:
        if P is not None:
            monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", str(P))
        got = batch(lib, mlhip, cp, group, True, pts, scs, False, lengths)
        assert [i for i in range(9) if got[i] != plain[i]] == [4], (name, group, P)
        rc, host = host_batch(hbe, cp, group, P or 4, pts, scs, lengths, False)
        assert rc == 0 and got == host, (name, group, P)
        monkeypatch.setenv("MLHIP_MSM_BATCH_ENDO", "0")
        assert batch(lib, mlhip, cp, group, True, pts, scs, False, lengths) == plain
        monkeypatch.delenv("MLHIP_MSM_BATCH_ENDO")
    if group == 2:  # no split chunk is compiled for G2 at P = 8: the plain chunk kernel
        monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", "8")
        assert batch(lib, mlhip, cp, group, True, pts, scs, False, lengths) == plain


@pytest.mark.parametrize("cid,group", [(1, 1), (2, 1), (0, 2), (1, 2), (2, 2)])
def test_device_form_on_a_busy_stream(lib, mlhip, delay, cid, group):
    """the _device form with the promise through the scenario of tests/test_stream_order_gpu.py: inputs still being produced
    on the stream, outputs overwritten right behind the call, the stream still busy when the call returns"""
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
    outcome = S.run_scenario(lib, mlhip, MsmBatchSubgroup(cid, group), torch.cuda.Stream(), delay, lines.append,
                             "msm-batch-subgroup-g%d-%s" % (group, S.NAMES[cid]))
    assert outcome.busy and lines


@pytest.mark.parametrize("name", list(CURVES))
def test_python_mirror(lib, mlhip, name):
    """MultiScalarMulBatchSubgroup / MultiScalarMulG2BatchSubgroup of mathlib_amd/driver.py equal the plain batch mirrors and
    the single MultiScalarMul on multiples of the generators, with the length rules of the plain mirrors"""
    from conftest import load_golden
    from mathlib_amd.driver import Curve

    cp = curve(name)
    cv = Curve(cp.curve_id)
    rng = random.Random("subgroup-mirror/" + name)
    co = load_golden(name)["g2_gen_coords"]  # (the mirror has no built-in BLS12-377 G2 generator)
    g2 = cv.NewG2FromCoords((int(co[0][0]), int(co[0][1])), (int(co[1][0]), int(co[1][1])))
    zr = [cv.NewRandomZr(rng.randrange) for _ in range(9)] + [cv.NewZrFromInt(-1), cv.GroupOrder, cv.NewZrFromInt(0)]
    for gen, fast, slow, single in ((cv.GenG1(), cv.MultiScalarMulBatchSubgroup, cv.MultiScalarMulBatch, cv.MultiScalarMul),
                                    (g2, cv.MultiScalarMulG2BatchSubgroup, cv.MultiScalarMulG2Batch, cv.MultiScalarMulG2)):
        pts = [gen.Mul(cv.NewZrFromInt(rng.randrange(1, cp.r))) for _ in range(11)] + [gen]
        a_lists = [pts[:3], [], pts[3:4], pts[4:12], pts[:2], pts[5:7]]
        b_lists = [zr[:3], [], zr[3:4], zr[4:12], zr[:3], zr[5:7]]  # segment 4: more scalars than points -> identity
        got = fast(a_lists, b_lists)
        assert [p.raw for p in got] == [p.raw for p in slow(a_lists, b_lists)]
        assert [p.raw for p in slow(a_lists, b_lists, subgroup=True)] == [p.raw for p in got]
        assert got[0].Equals(single(a_lists[0], b_lists[0])) and got[1].IsInfinity() and got[4].IsInfinity()
        assert fast([], []) == []
        with pytest.raises(IndexError):
            fast([pts[:3]], [zr[:2]])
        with pytest.raises(ValueError):
            fast([pts[:3]], [])
