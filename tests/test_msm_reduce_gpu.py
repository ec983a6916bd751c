"""The bucket reduction (msm_reduce.h: chunk sums, the W x nsel half / bit-masked sums, the group combine of folded plans)
through every path the build has, at the geometries where its index arithmetic can go wrong, against cref.msm -- bit-exact.

Paths: the default (carry-free quads for G1, carry-free lane pairs for G2), the test build's boundary-form quads / lane pairs
(MLHIP_REDUCE32) and one point per lane (MLHIP_REDUCE_ONE_LANE, G1), the Edwards reduction (BLS12-377 G1 with the SRS
promise) and the combine of a folded handle (shifted-base tables).  Geometries (window_c, MLHIP_CHUNK_LOG2): (5, 4) T = 1
(nb = 0, nsel = 4, the second half list empty), (5, 3) T = 2, (5, 1) L = 2 (the chunk loop runs once before the final
addition), (16, 3) T = 4096 (half a list exceeds a block's lane groups: the strided loop runs more than once and the upper
half of the lane pairs is full when it hands its sums over).  Only switches that exist are used: the tests pin behaviour."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
GEOMETRIES = [(5, 4), (5, 3), (5, 1), (16, 3)]  # (window_c, MLHIP_CHUNK_LOG2)
N_RANDOM = 240

_INPUTS = {}


def _scalar_rows(values):
    return np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for v in values], dtype=np.uint64)


def _inputs(curve, group):
    """(curve id, point bytes, points, scalars as bytes, n, expected), computed once per curve and group.  240 distinct points
    under 252-bit scalars (2^15 buckets per window at c = 16: most stay empty; 16 at c = 5: all collide), among them points at
    infinity, then pairs with small scalars that put the same point, or P beside -P, into neighbouring buckets of one chunk
    (the chunk loop meets acc = b[i] and acc = -b[i]) and into the same place of neighbouring chunks, for chunks of 2, 8 and
    16 buckets (the tree meets A[t] = +-A[t + 1]; w0 = acc after an empty bucket is a doubling too)."""
    key = (curve, group)
    if key not in _INPUTS:
        from oracle import cref
        from oracle import pyref as R

        cid = load_golden(curve)["curve_id"]
        r = R.CURVES[curve].r
        rng = np.random.default_rng(1000 * group + cid)
        n0 = N_RANDOM
        base = cref.gen_points(cid, group, 4242 + cid, 99 + group, n0)
        ptb = len(base) // n0
        pt = [base[i * ptb : (i + 1) * ptb] for i in range(n0)]
        for i in (3, 77, n0 - 1):
            pt[i] = bytes(ptb)  # infinity
        vals = [int.from_bytes(rng.bytes(32), "little") >> 4 for _ in range(n0)]
        vals[5] = 0
        vals[6] = 1
        vals[7] = r - 1
        pt[9], vals[9] = pt[8], vals[8]  # the same pair twice: every bucket addition of it is a doubling
        pt[11], vals[11] = cref.point_mul(cid, group, pt[10], r - 1), vals[10]  # P beside -P under one scalar: empty again
        k = 20
        for L in (2, 8, 16):
            for d in (1, 2, L):  # bucket d - 1 of chunk 0 and its neighbours
                P, Q, S = pt[k], pt[k + 1], pt[k + 2]
                k += 3
                pt += [P, P, Q, cref.point_mul(cid, group, Q, r - 1), S, S]
                vals += [d, d + 1, d + 2, d + 3, d + 4 * L, d + 5 * L]
                pt += [cref.point_mul(cid, group, S, r - 1)]
                vals += [d + 7 * L]
        n = len(pt)
        pts = b"".join(pt)
        sc = _scalar_rows(vals)
        _INPUTS[key] = (cid, ptb, pts, sc.tobytes(), n, cref.msm(cid, group, pts, sc, n, False, 0, 8))
    return _INPUTS[key]


def _host_msm(lib, mlhip, cid, group, pts, scs, n, window_c, ptb):
    out = ctypes.create_string_buffer(ptb)
    fn = lib.mlhip_msm_g1 if group == 1 else lib.mlhip_msm_g2
    mlhip.check(fn(cid, pts, scs, 0, n, window_c, out))
    return out.raw


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.mark.parametrize("curve", CURVES)
# (G2 has no one-lane reduction: the switch is read for G1 only)
@pytest.mark.parametrize("group,path", [(1, "default"), (1, "MLHIP_REDUCE32"), (1, "MLHIP_REDUCE_ONE_LANE"), (2, "default"),
                                        (2, "MLHIP_REDUCE32")])
def test_reduction_paths_at_edge_geometries(lib, mlhip, curve, group, path, monkeypatch):
    cid, ptb, pts, scs, n, want = _inputs(curve, group)
    monkeypatch.setenv("MLHIP_NO_PLAN_CACHE", "1")  # the knobs are read when a plan is created: no pooled plan
    if path != "default":
        monkeypatch.setenv(path, "1")  # (routes the rest of the test through the test build)
    for window_c, chunk_log2 in GEOMETRIES:
        monkeypatch.setenv("MLHIP_CHUNK_LOG2", str(chunk_log2))
        got = _host_msm(lib, mlhip, cid, group, pts, scs, n, window_c, ptb)
        assert got == want, (curve, group, path, window_c, chunk_log2)


@pytest.mark.parametrize("chunk_log2", [3, 1])
def test_edwards_reduction(lib, mlhip, chunk_log2, monkeypatch):
    """BLS12-377 G1 with the SRS promise: buckets, chunk sums and masked sums in extended twisted Edwards coordinates, the
    W x nsel sums converted back.  The promise is honoured only above 32768 buckets (below, one bucket per quad of lanes on
    XYZZ), so the geometries are c = 16 with chunks of 8 (T = 4096) and of 2 (L = 2, T = 16384)."""
    import torch

    cid, ptb, pts, scs, n, want = _inputs("BLS12-377", 1)
    monkeypatch.setenv("MLHIP_CHUNK_LOG2", str(chunk_log2))
    dev = torch.device("cuda", 0)
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(scs), dtype=torch.uint8).to(dev)
    plan = mlhip.MsmPlan(cid, 1, n, 16)
    try:
        plan.assume_srs(True)
        assert plan.run(dp.data_ptr(), ds.data_ptr(), n, False, torch.cuda.current_stream().cuda_stream) == want
        assert plan.timings()["edwards"] == 1.0
    finally:
        plan.close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fold_c", [17, 20])
def test_folded_handle_group_combine(lib, mlhip, curve, group, fold_c, monkeypatch):
    """The combine of a folded handle: groups of 32768 buckets, so 17-bit digits give W = 2 groups (the smallest combine) and
    20-bit digits, the widest the library takes, W = 16.  (BLS12-377 G1: the table is in the subgroup, so the sums that are
    combined come from the Edwards reduction.)"""
    cid, ptb, pts, scs, n, want = _inputs(curve, group)
    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", str(fold_c))
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_bases_create(cid, group, pts, n, 0, ctypes.byref(h)))
    try:
        out = ctypes.create_string_buffer(ptb)
        mlhip.check(lib.mlhip_bases_msm(h, scs, 0, n, out))
        t = mlhip.plan_timings(lib, lib.mlhip_bases_plan(h))
        assert t["tables"] == 1.0 and t["window_c"] == fold_c, t
        assert out.raw == want, (curve, group, fold_c)
    finally:
        mlhip.check(lib.mlhip_bases_destroy(h))
