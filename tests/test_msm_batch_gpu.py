"""The batched MSM on the GPU (mlhip_msm_batch / mlhip_msm_batch_device, mathlib_amd/csrc/msm_batch.h): byte equality with
cref.msm for every segment -- every curve, G1 and G2, mixed segment lengths in random order, Montgomery and plain
non-canonical scalars, the degenerate pairs of tests/msm_batch_cases.py inside one chunk -- the default chunk length
against P = 1 (one product per lane), against mlhip_msm_g1 / _g2 of single segments, 2^16 segments of 4 pairs, the
device form on a non-default stream, argument checks, and the Python mirrors."""
import ctypes
import random

import pytest

from msm_batch_cases import CURVES, curve, edge_segments, expected, point_bytes, random_segments

pytestmark = pytest.mark.gpu

CHUNKS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def mixed_lengths(seed: str, P: int = 4):
    """about 300 segments of lengths {0, 1, 2, 3, P, P + 1, 17, 64, 1000} in random order (1000 twice)"""
    rnd = random.Random(seed)
    small = [0, 1, 2, 3, P, P + 1, 17]
    lengths = [1000, 1000] + [64] * 8 + [rnd.choice(small) for _ in range(290)]
    rnd.shuffle(lengths)
    return lengths


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_mixed_segments_match_cref(lib, mlhip, name, group):
    cp = curve(name)
    lengths = mixed_lengths("gpu-mixed/%s/%d" % (name, group))
    pts, scs, lengths = random_segments(cp, group, lengths, "gpu-mixed/%s/%d" % (name, group))
    for mont in (False, True):
        got = mlhip.msm_batch(cp.curve_id, group, pts, scs, mont, lengths)
        exp = expected(cp, group, pts, scs, lengths, mont)
        bad = [i for i in range(len(exp)) if got[i] != exp[i]]
        assert not bad, (name, group, mont, bad[:10], [lengths[i] for i in bad[:10]])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_degenerate_pairs_inside_one_chunk(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    for pad in (0, 1, 3):
        pts, scs, lengths = edge_segments(cp, group, "gpu-edge/%s/%d" % (name, group), pad)
        for mont in (False, True):
            exp = expected(cp, group, pts, scs, lengths, mont)
            for P in CHUNKS:
                monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", str(P))
                got = mlhip.msm_batch(cp.curve_id, group, pts, scs, mont, lengths)
                assert got == exp, (name, group, pad, mont, P, [i for i in range(len(exp)) if got[i] != exp[i]])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_default_chunk_equals_one_product_per_lane(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    lengths = mixed_lengths("gpu-p1/%s/%d" % (name, group))[:120]
    pts, scs, lengths = random_segments(cp, group, lengths, "gpu-p1/%s/%d" % (name, group))
    monkeypatch.delenv("MLHIP_MSM_BATCH_CHUNK", raising=False)
    default = mlhip.msm_batch(cp.curve_id, group, pts, scs, True, lengths)
    for P in (1, 2, 8):
        monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", str(P))
        assert mlhip.msm_batch(cp.curve_id, group, pts, scs, True, lengths) == default, P
    monkeypatch.setenv("MLHIP_MSM_BATCH_CHUNK", "3")  # not a compiled length: the default
    assert mlhip.msm_batch(cp.curve_id, group, pts, scs, True, lengths) == default


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_segments_equal_single_msm_calls(lib, mlhip, name, group):
    cp = curve(name)
    lengths = [5, 1000, 0, 64, 2, 33]
    pts, scs, lengths = random_segments(cp, group, lengths, "gpu-single/%s/%d" % (name, group))
    got = mlhip.msm_batch(cp.curve_id, group, pts, scs, False, lengths)
    ps = point_bytes(cp, group)
    fn = lib.mlhip_msm_g1 if group == 1 else lib.mlhip_msm_g2
    o = 0
    for i, m in enumerate(lengths):
        out = ctypes.create_string_buffer(ps)
        mlhip.check(fn(cp.curve_id, pts[o * ps : (o + m) * ps], scs[32 * o : 32 * (o + m)], 0, m, 0, out))
        assert got[i] == out.raw, (name, group, i, m)
        o += m


def test_bls12_381_g1_65536_segments_of_4(lib, mlhip):
    """2^16 segments of 4 pairs through the device form: every output against cref"""
    import torch

    cp = curve("BLS12-381")
    K, m = 1 << 16, 4
    pts, scs, lengths = random_segments(cp, 1, [m] * K, "gpu-64k")
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    ds = torch.frombuffer(bytearray(scs), dtype=torch.uint8).cuda()
    out = torch.zeros(K * 96, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    mlhip.check(lib.mlhip_msm_batch_device(cp.curve_id, 1, dp.data_ptr(), ds.data_ptr(), 0, mlhip.batch_offsets(lengths), K,
                                           out.data_ptr(), st.cuda_stream))
    st.synchronize()
    got = out.cpu().numpy().tobytes()
    exp = b"".join(expected(cp, 1, pts, scs, lengths, False))
    assert got == exp, [i for i in range(K) if got[96 * i : 96 * (i + 1)] != exp[96 * i : 96 * (i + 1)]][:10]


@pytest.mark.parametrize("group", [1, 2])
def test_device_form_on_a_non_default_stream(lib, mlhip, group):
    import torch

    cp = curve("BN254")
    lengths = mixed_lengths("gpu-stream/%d" % group)[:100]
    pts, scs, lengths = random_segments(cp, group, lengths, "gpu-stream/%d" % group)
    ps = point_bytes(cp, group)
    K = len(lengths)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
        ds = torch.frombuffer(bytearray(scs), dtype=torch.uint8).cuda()
        out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
        mlhip.check(lib.mlhip_msm_batch_device(cp.curve_id, group, dp.data_ptr(), ds.data_ptr(), 1, mlhip.batch_offsets(lengths), K,
                                               out.data_ptr(), s.cuda_stream))
        got = out.cpu().numpy().tobytes()  # on s: ordered after the batch
    s.synchronize()
    assert got == b"".join(expected(cp, group, pts, scs, lengths, True))


def test_empty_batch_and_malformed_offsets(lib, mlhip):
    cp = curve("BLS12-381")
    pts, scs, lengths = random_segments(cp, 1, [2, 3], "gpu-args")
    out = ctypes.create_string_buffer(2 * 96)
    # k = 0: nothing to do, nothing touched (null pointers are fine)
    assert lib.mlhip_msm_batch(cp.curve_id, 1, None, None, 0, None, 0, None) == 0
    assert lib.mlhip_msm_batch_device(cp.curve_id, 1, None, None, 0, None, 0, None, None) == 0
    assert mlhip.msm_batch(cp.curve_id, 1, b"", b"", False, []) == []

    def offs(*v):
        return (ctypes.c_uint64 * len(v))(*v)

    einval = -1
    for bad in (offs(0, 3, 2), offs(1, 3, 5), offs(0, 5, 4)):
        assert lib.mlhip_msm_batch(cp.curve_id, 1, pts, scs, 0, bad, 2, out) == einval
        assert lib.mlhip_msm_batch_device(cp.curve_id, 1, pts, scs, 0, bad, 2, out, None) == einval
    assert lib.mlhip_msm_batch(cp.curve_id, 1, pts, scs, 0, None, 2, out) == einval
    assert lib.mlhip_msm_batch(cp.curve_id, 1, None, scs, 0, offs(0, 2, 5), 2, out) == einval
    assert lib.mlhip_msm_batch(cp.curve_id, 1, pts, None, 0, offs(0, 2, 5), 2, out) == einval
    assert lib.mlhip_msm_batch(cp.curve_id, 1, pts, scs, 0, offs(0, 2, 5), 2, None) == einval
    assert lib.mlhip_msm_batch(cp.curve_id, 3, pts, scs, 0, offs(0, 2, 5), 2, out) == einval
    assert lib.mlhip_msm_batch(9, 1, pts, scs, 0, offs(0, 2, 5), 2, out) == einval
    # all segments empty: null inputs are fine, every output is the point at infinity
    assert lib.mlhip_msm_batch(cp.curve_id, 1, None, None, 0, offs(0, 0, 0), 2, out) == 0
    assert out.raw == bytes(2 * 96)
    # and a well-formed call still works after the refusals
    assert lib.mlhip_msm_batch(cp.curve_id, 1, pts, scs, 0, offs(0, 2, 5), 2, out) == 0
    assert [out.raw[:96], out.raw[96:]] == expected(cp, 1, pts, scs, lengths, False)


@pytest.mark.parametrize("name", CURVES)
def test_python_mirrors(lib, name):
    from mathlib_amd.driver import G2, Curve
    from oracle import cref

    cp = curve(name)
    cv = Curve(cp.curve_id)
    rng = random.Random("mirror/" + name)
    g = cv.GenG1()
    pts1 = [g.Mul(cv.NewZrFromInt(rng.randrange(1, cp.r))) for _ in range(12)]
    zr = [cv.NewRandomZr(rng.randrange) for _ in range(12)]
    a_lists = [pts1[:3], [], pts1[3:4], pts1[4:11], pts1[:2], pts1[5:7]]
    b_lists = [zr[:3], [], zr[3:4], zr[4:11], zr[:3], zr[5:7]]  # segment 4: more scalars than points -> identity
    got = cv.MultiScalarMulBatch(a_lists, b_lists)
    assert len(got) == len(a_lists)
    for x, a, b in zip(got, a_lists, b_lists):
        assert x.Equals(cv.MultiScalarMul(a, b))
    assert got[4].IsInfinity() and got[1].IsInfinity()
    with pytest.raises(IndexError):
        cv.MultiScalarMulBatch([pts1[:3]], [zr[:2]])
    with pytest.raises(ValueError):
        cv.MultiScalarMulBatch([pts1[:3]], [])
    assert cv.MultiScalarMulBatch([], []) == []
    e, f = zr[:6], zr[6:12]
    gs, qs = pts1[:6], pts1[6:12]
    m2 = cv.Mul2Batch(gs, e, qs, f)
    for i in range(6):
        assert m2[i].Equals(gs[i].Mul2(e[i], qs[i], f[i]))
    with pytest.raises(ValueError):
        cv.Mul2Batch(gs, e[:5], qs, f)
    raw2 = cref.gen_points(cp.curve_id, 2, 0xA11CE, 0xB0B, 6)
    ps2 = point_bytes(cp, 2)
    pts2 = [G2(raw2[i * ps2 : (i + 1) * ps2], cv) for i in range(6)]
    a2 = [pts2[:2], pts2[2:6], [], pts2[:1]]
    b2 = [zr[:2], zr[2:6], zr[:1], zr[:1]]
    got2 = cv.MultiScalarMulG2Batch(a2, b2)
    for x, a, b in zip(got2, a2, b2):
        assert x.Equals(cv.MultiScalarMulG2(a, b))
    assert got2[2].IsInfinity()
    with pytest.raises(IndexError):
        cv.MultiScalarMulG2Batch([pts2[:3]], [zr[:1]])
