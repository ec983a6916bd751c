"""Short-scalar MSMs on the GPU (include/mlhip_bits.h; here through the binding's functions of the same names, which pack the
scalar width into window_c as the header's inline functions do): mlhip_msm_bits and plans made by mlhip_msm_plan_create_bits, through every entry point a
plan runs through (one pass, tiles, streamed segments, shared launch, the SRS promise, the second implementations, the
plan pool), against oracle.cref's MSM over the MASKED scalars (s mod r) mod 2^bits -- bit-exact."""
import ctypes
import random

import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
FR_BITS = {"BN254": 254, "BLS12-381": 255, "BLS12-377": 253}
R256 = 1 << 256


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def eff_bits(curve, bits):
    return FR_BITS[curve] if (bits == 0 or bits >= FR_BITS[curve]) else bits


def windows(curve, bits, c):
    """(c', W) of a plan over `bits`-bit scalars asked for width c (include/mlhip.h)"""
    b = eff_bits(curve, bits)
    W = -(-(b + 1) // c)
    return (c if b == FR_BITS[curve] else max(4, -(-(b + 1) // W))), W


_POINTS = {}


def points(curve, group, n):
    """n points: every 64th a duplicate of point 0, two infinities, one -P behind its P -- made once per (curve, group, n)"""
    key = (curve, group, n)
    if key not in _POINTS:
        from oracle import cref
        from oracle import pyref as R

        cp = R.CURVES[curve]
        fb = cp.fp_bytes
        sz = 2 * group * fb
        pts = bytearray(cref.gen_points(cp.curve_id, group, 9001 + group, 313, n))
        for i in range(64, n, 64):
            pts[i * sz : (i + 1) * sz] = pts[0:sz]
        if n > 12:
            pts[7 * sz : 8 * sz] = bytes(sz)
            pts[(n - 1) * sz : n * sz] = bytes(sz)
            neg = bytearray(pts[10 * sz : 11 * sz])
            for k in range(group, 2 * group):  # the y coordinate: one (G1) or two (G2) field elements, Montgomery form
                y = int.from_bytes(neg[k * fb : (k + 1) * fb], "little")
                neg[k * fb : (k + 1) * fb] = ((cp.p - y) % cp.p).to_bytes(fb, "little")
            pts[11 * sz : 12 * sz] = neg
        _POINTS[key] = bytes(pts)
    return _POINTS[key]


def scalars(curve, n, bits, mont, seed=0, promise=False):
    """(the bytes handed to the library, the masked canonical values as bytes for the oracle).  Random values below 2^bits with
    the planted ones of the issue: 0, 1, 2^bits - 1, 2^(bits-1), an all-ones window at each end, and -- unless `promise` -- the
    promise-breakers r - 1 and 2^256 - 1 (mont: every row is in Montgomery form; the last breaker is the raw row 2^256 - 1)"""
    from oracle import pyref as R

    r = R.CURVES[curve].r
    b = eff_bits(curve, bits)
    rnd = random.Random("msm-bits/%s/%d/%d/%d" % (curve, n, b, seed))
    vals = [rnd.getrandbits(b) for _ in range(n)]
    if n >= 12:
        w = min(16, b)
        vals[0:6] = [0, 1, (1 << b) - 1, 1 << (b - 1), (1 << w) - 1, ((1 << w) - 1) << (b - w)]
        vals[11] = vals[10]  # (the point at 11 is minus the point at 10)
        if not promise:
            vals[8], vals[9] = r - 1, R256 - 1
    rinv = pow(R256, -1, r)
    raw, canon = [], []
    for i, v in enumerate(vals):
        if mont and not promise and n >= 12 and i == 9:
            raw.append(R256 - 1)  # not the image of anything: still a defined input
            canon.append((R256 - 1) * rinv % r)
        elif mont:
            raw.append((v % r) * R256 % r)
            canon.append(v % r)
        else:
            raw.append(v)
            canon.append(v % r)
    mask = (1 << b) - 1
    return (b"".join(v.to_bytes(32, "little") for v in raw), b"".join((v & mask).to_bytes(32, "little") for v in canon))


def oracle(cid, group, pts, masked, n):
    from oracle import cref

    return cref.msm(cid, group, pts, masked, n, False, 0, 8)


def msm_bits(lib, mlhip, cid, group, pts, sc, mont, bits, n, c):
    g1b, g2b = mlhip.sizes(cid)[1:3]
    out = ctypes.create_string_buffer(g1b if group == 1 else g2b)
    mlhip.check(mlhip.mlhip_msm_bits(lib, cid, group, pts, sc, 1 if mont else 0, bits, n, c, out))
    return out.raw


N_HOST = 1500


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_host_form(lib, mlhip, curve, group):
    """mlhip_msm_bits at every width class (below, at and across a word and a window; fr_bits - 1; the three spellings of
    full width) and window width, Montgomery rows on one width per curve, n = 0 with null pointers and n = 1"""
    cid = load_golden(curve)["curve_id"]
    fr = FR_BITS[curve]
    pts = points(curve, group, N_HOST)
    mont_bits = {"BN254": 33, "BLS12-381": 64, "BLS12-377": 127}[curve]
    for bits in (1, 7, 31, 32, 33, 64, 127, 128, 129, fr - 1, fr, 0, 256):
        for mont in (False, True) if bits == mont_bits else (False,):
            sc, masked = scalars(curve, N_HOST, bits, mont)
            want = oracle(cid, group, pts, masked, N_HOST)
            for c in (0, 4, 8, 13, 16):
                assert msm_bits(lib, mlhip, cid, group, pts, sc, mont, bits, N_HOST, c) == want, (curve, group, bits, mont, c)
    sz = len(pts) // N_HOST
    assert msm_bits(lib, mlhip, cid, group, None, None, False, 64, 0, 0) == bytes(sz)
    one_pts = points(curve, group, 1)
    for bits in (1, 64, 0):
        sc, masked = scalars(curve, 1, bits, False, seed=5)
        assert msm_bits(lib, mlhip, cid, group, one_pts, sc, False, bits, 1, 0) == oracle(cid, group, one_pts, masked, 1)


def test_full_width_is_the_old_call(lib, mlhip):
    """scalar_bits = 0 / fr_bits / 256: the bytes of mlhip_msm_g1 / _g2, and the geometry of mlhip_msm_plan_create"""
    curve = "BLS12-377"
    cid = load_golden(curve)["curve_id"]
    for group, fn in ((1, lib.mlhip_msm_g1), (2, lib.mlhip_msm_g2)):
        pts = points(curve, group, N_HOST)
        sc, _ = scalars(curve, N_HOST, 0, False)
        out = ctypes.create_string_buffer(len(pts) // N_HOST)
        mlhip.check(fn(cid, pts, sc, 0, N_HOST, 0, out))
        for bits in (0, FR_BITS[curve], 256):
            assert msm_bits(lib, mlhip, cid, group, pts, sc, False, bits, N_HOST, 0) == out.raw
    for c in (0, 13, 18):
        old = mlhip.MsmPlan(cid, 1, 5000, c)
        for bits in (FR_BITS[curve], 255, 256):
            new = mlhip.MsmPlan(cid, 1, 5000, c, bits)
            assert new.window() == old.window() and new.scalar_bits() == old.scalar_bits() == FR_BITS[curve]
            new.close()
        old.close()


def test_einval(lib, mlhip):
    cid = load_golden("BLS12-381")["curve_id"]
    pts = points("BLS12-381", 1, N_HOST)
    sc, _ = scalars("BLS12-381", N_HOST, 64, False)
    out = ctypes.create_string_buffer(len(pts) // N_HOST)
    for bits in (-1, 257):
        assert mlhip.mlhip_msm_bits(lib, cid, 1, pts, sc, 0, bits, N_HOST, 0, out) == mlhip.EINVAL
        h = ctypes.c_void_p(1)
        assert mlhip.mlhip_msm_plan_create_bits(lib, cid, 1, 1000, 0, bits, ctypes.byref(h)) == mlhip.EINVAL
        assert not h.value  # the plan pointer is left NULL
    assert mlhip.mlhip_msm_bits(lib, cid, 3, pts, sc, 0, 64, N_HOST, 0, out) == mlhip.EINVAL
    h = ctypes.c_void_p(1)
    assert mlhip.mlhip_msm_bits(lib, 7, 1, pts, sc, 0, 64, N_HOST, 0, out) == mlhip.EINVAL and b"unknown curve id" in lib.mlhip_last_error()
    assert lib.mlhip_set_device(99) == mlhip.EINVAL  # (another error text in between)
    assert mlhip.mlhip_msm_plan_create_bits(lib, 7, 1, 1000, 0, 64, ctypes.byref(h)) == mlhip.EINVAL
    assert b"unknown curve id" in lib.mlhip_last_error() and not h.value
    assert mlhip.mlhip_msm_plan_scalar_bits(lib, None)[0] == mlhip.EINVAL


def test_packed_window_is_rejected_everywhere_else(lib, mlhip):
    """MLHIP_WINDOW_BITS is understood by mlhip_msm_plan_create / _g1 / _g2 only: the resident-bases handles, the explicit device
    list and the shared-scalar call reject it as they reject any window_c above 20 -- no handle, nothing written -- and a
    handle made with a plain window_c still sums at full width"""
    import torch

    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n = N_HOST
    p1, p2 = points(curve, 1, n), points(curve, 2, n)
    sc, full = scalars(curve, n, 0, False)
    dev0 = (ctypes.c_int * 1)(0)
    dp = torch.frombuffer(bytearray(p1), dtype=torch.uint8).cuda()
    for packed in (mlhip.window_bits(16, 64), mlhip.window_bits(0, 64), mlhip.window_bits(16, 1), 272):
        o1, o2 = ctypes.create_string_buffer(b"\x5a" * 96, 96), ctypes.create_string_buffer(b"\x5a" * 192, 192)
        for group, pts in ((1, p1), (2, p2)):
            h = ctypes.c_void_p()
            assert lib.mlhip_bases_create(cid, group, pts, n, packed, ctypes.byref(h)) == mlhip.EINVAL and not h.value, (packed, group)
            assert lib.mlhip_bases_create_multi(cid, group, dev0, 1, pts, n, packed, ctypes.byref(h)) == mlhip.EINVAL and not h.value
            assert lib.mlhip_msm_multi(cid, group, dev0, 1, pts, sc, 0, n, packed, o1 if group == 1 else o2) == mlhip.EINVAL
        h = ctypes.c_void_p()
        assert lib.mlhip_bases_create_device(cid, 1, dp.data_ptr(), n, packed, ctypes.byref(h)) == mlhip.EINVAL and not h.value
        assert lib.mlhip_msm_g1g2(cid, p1, p2, sc, 0, n, packed, o1, o2) == mlhip.EINVAL
        assert o1.raw == b"\x5a" * 96 and o2.raw == b"\x5a" * 192
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_bases_create(cid, 1, p1, n, 16, ctypes.byref(h)))
    try:
        assert mlhip.mlhip_msm_plan_scalar_bits(lib, lib.mlhip_bases_plan(h)) == (0, FR_BITS[curve])
        out = ctypes.create_string_buffer(96)
        mlhip.check(lib.mlhip_bases_msm(h, sc, 0, n, out))
        assert out.raw == oracle(cid, 1, p1, full, n)
    finally:
        lib.mlhip_bases_destroy(h)


N_PLAN = 5000


@pytest.mark.parametrize("curve,group", [(c, 1) for c in CURVES] + [("BLS12-381", 2)])
def test_plan_route(lib, mlhip, curve, group, monkeypatch):
    """MsmPlan(..., scalar_bits) over device tensors: one pass and tiles (the sort-ahead records inherit the width), the
    plan reused with a shorter n, profiling, out_xyzz; the plan reports c' and its short W"""
    import torch

    cid = load_golden(curve)["curve_id"]
    pts = points(curve, group, N_PLAN)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    for bits in (33, 128):
        sc, masked = scalars(curve, N_PLAN, bits, False)
        ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
        want = oracle(cid, group, pts, masked, N_PLAN)
        want_head = oracle(cid, group, pts, masked, 3001)
        for c in (8, 13):
            plan = mlhip.MsmPlan(cid, group, N_PLAN, c, bits)
            full = mlhip.MsmPlan(cid, group, N_PLAN, c)
            try:
                ce, W = windows(curve, bits, c)
                assert plan.window() == (ce, W), (bits, c, plan.window())
                t = plan.timings()
                assert t["window_c"] == ce and t["digits_per_scalar"] == W == -(-(bits + 1) // c)
                assert W < full.window()[1]  # strictly fewer windows than the full-width plan
                assert mlhip.mlhip_msm_plan_scalar_bits(lib, plan._h) == (0, bits)
                assert plan.scalar_bits() == bits and full.scalar_bits() == FR_BITS[curve]
                plan.set_profiling(True)
                for tile in ("10", "12", "0"):  # 5 tiles (ragged), 2 tiles, one pass
                    monkeypatch.setenv("MLHIP_TILE_LOG2", tile)
                    assert plan.run(dp.data_ptr(), ds.data_ptr(), N_PLAN, False, st) == want, (curve, group, bits, c, tile)
                    t = plan.timings()
                    assert t["accumulate"] > 0 and t["device_total"] >= t["accumulate"], (tile, t)
                    assert plan.run(dp.data_ptr(), ds.data_ptr(), 3001, False, st) == want_head, (curve, group, bits, c, tile)
                aff, xyzz = plan.run(dp.data_ptr(), ds.data_ptr(), N_PLAN, False, st, want_xyzz=True)
                assert aff == want and len(xyzz) == 2 * len(aff) and any(xyzz)
            finally:
                plan.close()
                full.close()


@pytest.mark.parametrize("curve,group", [(c, 1) for c in CURVES] + [("BLS12-381", 2)])
def test_streamed_host_form(lib, mlhip, curve, group, monkeypatch):
    """mlhip_msm_bits in segments (MLHIP_STREAM_SEGMENTS) and in one pass; an all-equal scalar vector puts long buckets in
    every segment"""
    cid = load_golden(curve)["curve_id"]
    n, bits = 4000, 65
    pts = points(curve, group, n)
    sc, masked = scalars(curve, n, bits, False)
    same = (0x1F0E1D2C3B4A59687 & ((1 << bits) - 1)).to_bytes(32, "little") * n
    cases = [(sc, oracle(cid, group, pts, masked, n)), (same, oracle(cid, group, pts, same, n))]
    monkeypatch.setenv("MLHIP_NO_PLAN_CACHE", "1")
    for seg in ("0", "3"):
        monkeypatch.setenv("MLHIP_STREAM_SEGMENTS", seg)
        for c in (8, 16):
            for k, (s, want) in enumerate(cases):
                assert msm_bits(lib, mlhip, cid, group, pts, s, False, bits, n, c) == want, (curve, group, seg, c, k)


def test_shared_launch(lib, mlhip, monkeypatch):
    """mlhip_msm_launch_shared on short plans: equal widths share one sort and give the bytes of the two plans run separately;
    plans of different widths (64 bits and full) run one after the other and are each right"""
    import torch

    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n = N_PLAN
    p1, p2 = points(curve, 1, n), points(curve, 2, n)
    sc, masked = scalars(curve, n, 64, False)
    full_sc, full_masked = scalars(curve, n, 0, False)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    d1 = torch.frombuffer(bytearray(p1), dtype=torch.uint8).to(dev)
    d2 = torch.frombuffer(bytearray(p2), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    dfull = torch.frombuffer(bytearray(full_sc), dtype=torch.uint8).to(dev)
    want1, want2 = oracle(cid, 1, p1, masked, n), oracle(cid, 2, p2, masked, n)
    a, b = mlhip.MsmPlan(cid, 1, n, 13, 64), mlhip.MsmPlan(cid, 2, n, 13, 64)
    wide = mlhip.MsmPlan(cid, 2, n, 13)
    try:
        for tile in ("0", "11"):
            monkeypatch.setenv("MLHIP_TILE_LOG2", tile)
            sep1 = a.run(d1.data_ptr(), ds.data_ptr(), n, False, st)
            sep2 = b.run(d2.data_ptr(), ds.data_ptr(), n, False, st)
            a.launch_shared(b, d1.data_ptr(), d2.data_ptr(), ds.data_ptr(), n, False, st)
            assert a.finish() == sep1 == want1 and b.finish() == sep2 == want2, tile
            # a 64-bit G1 plan beside a full-width G2 plan over full-width scalars: G1 masked, G2 not
            mask64 = b"".join(full_masked[32 * i : 32 * i + 8] + bytes(24) for i in range(n))
            a.launch_shared(wide, d1.data_ptr(), d2.data_ptr(), dfull.data_ptr(), n, False, st)
            assert a.finish() == oracle(cid, 1, p1, mask64, n), tile
            assert wide.finish() == oracle(cid, 2, p2, full_masked, n), tile
    finally:
        a.close()
        b.close()
        wide.close()


def test_srs_promise(lib, mlhip):
    """BLS12-377 G1, 128-bit scalars: with the SRS promise the short plan sums its buckets in twisted Edwards coordinates and
    gives the same bytes"""
    import torch

    curve = "BLS12-377"
    cid = load_golden(curve)["curve_id"]
    n, bits = N_PLAN, 128
    pts = points(curve, 1, n)
    sc, masked = scalars(curve, n, bits, False)
    want = oracle(cid, 1, pts, masked, n)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    for c in (13, 16):
        plan = mlhip.MsmPlan(cid, 1, n, c, bits)
        try:
            plain = plan.run(dp.data_ptr(), ds.data_ptr(), n, False, st)
            assert plain == want and plan.timings()["edwards"] == 0.0
            plan.assume_srs(True)
            assert plan.run(dp.data_ptr(), ds.data_ptr(), n, False, st) == plain, c
            assert plan.timings()["edwards"] == 1.0
        finally:
            plan.close()


@pytest.mark.parametrize("switch", ["MLHIP_ACC32", "MLHIP_LEGACY_SORT", "MLHIP_REDUCE_ONE_LANE", "MLHIP_REDUCE32", "MLHIP_NO_QUAD_ACC",
                                    "MLHIP_SCATTER_STAGED=0"])
def test_second_implementations(lib, mlhip, switch, monkeypatch):
    """the short width through the second implementations of every phase (the legacy digits path and the one-store-per-entry
    scatter take the width as an argument too); G2 for the two switches that have G2 forms"""
    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    name, _, value = switch.partition("=")
    monkeypatch.setenv(name, value or "1")
    monkeypatch.setenv("MLHIP_NO_PLAN_CACHE", "1")  # the switches are read when a plan is created: no pooled plan
    n, bits = N_HOST, 65
    for group in (1, 2) if name in ("MLHIP_ACC32", "MLHIP_REDUCE32") else (1,):
        pts = points(curve, group, n)
        sc, masked = scalars(curve, n, bits, False)
        want = oracle(cid, group, pts, masked, n)
        for c in (8, 16):
            assert msm_bits(lib, mlhip, cid, group, pts, sc, False, bits, n, c) == want, (switch, group, c)


def test_pool_keeps_widths_apart(lib, mlhip):
    """same (curve, n, c): a full-width call, a 40-bit call on the same full-width scalars, a full-width call again -- a pooled
    plan of one width never serves the other"""
    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n, c = N_HOST, 12
    pts = points(curve, 1, n)
    sc, full = scalars(curve, n, 0, False)
    sc2, full2 = scalars(curve, n, 0, False, seed=2)
    m40 = b"".join(full[32 * i : 32 * i + 5] + bytes(27) for i in range(n))
    out = ctypes.create_string_buffer(len(pts) // n)
    mlhip.check(lib.mlhip_msm_g1(cid, pts, sc, 0, n, c, out))
    assert out.raw == oracle(cid, 1, pts, full, n)
    short = msm_bits(lib, mlhip, cid, 1, pts, sc, False, 40, n, c)
    assert short == oracle(cid, 1, pts, m40, n) != out.raw
    mlhip.check(lib.mlhip_msm_g1(cid, pts, sc2, 0, n, c, out))
    assert out.raw == oracle(cid, 1, pts, full2, n)
    assert msm_bits(lib, mlhip, cid, 1, pts, sc, False, 40, n, c) == short


@pytest.mark.parametrize("curve", CURVES)
def test_size_that_fills_real_windows(lib, mlhip, curve):
    """2^14 points, 128 bits: every bucket of the nine 14/15-bit windows is in play"""
    cid = load_golden(curve)["curve_id"]
    n, bits = 1 << 14, 128
    pts = points(curve, 1, n)
    sc, masked = scalars(curve, n, bits, False)
    want = oracle(cid, 1, pts, masked, n)
    for c in (0, 16):
        assert msm_bits(lib, mlhip, cid, 1, pts, sc, False, bits, n, c) == want, (curve, c)


def test_python_driver_short_msm(lib, mlhip):
    """driver.Curve.MultiScalarMulShort / MultiScalarMulG2Short: the full-width result when the scalars keep the promise, the
    masked sum when they do not, MultiScalarMul's length rules"""
    from mathlib_amd.driver import Curve

    g = load_golden("BLS12-381")
    cv = Curve(g["curve_id"])
    co = g["g2_gen_coords"]
    gen2 = cv.NewG2FromCoords((int(co[0][0]), int(co[0][1])), (int(co[1][0]), int(co[1][1])))
    rnd = random.Random(64)
    n = 33
    g1s = [cv.GenG1().Mul(cv.NewZrFromInt(rnd.getrandbits(200))) for _ in range(n - 1)] + [cv.NewG1()]
    g2s = [gen2.Mul(cv.NewZrFromInt(rnd.getrandbits(200))) for _ in range(n)]
    small = [rnd.getrandbits(64) for _ in range(n)]
    zs = [cv.NewZrFromInt(v) for v in small]
    assert cv.MultiScalarMulShort(g1s, zs, 64).Equals(cv.MultiScalarMul(g1s, zs))
    assert cv.MultiScalarMulG2Short(g2s, zs, 64).Equals(cv.MultiScalarMulG2(g2s, zs))
    low = [cv.NewZrFromInt(v & 0xFFFFF) for v in small]
    assert cv.MultiScalarMulShort(g1s, zs, 20).Equals(cv.MultiScalarMul(g1s, low))
    assert cv.MultiScalarMulShort(g1s, zs, 0).Equals(cv.MultiScalarMul(g1s, zs))
    assert cv.MultiScalarMulShort(g1s[:3], zs[:5], 64).IsInfinity() and cv.MultiScalarMulG2Short([], [], 64).IsInfinity()
    with pytest.raises(IndexError):
        cv.MultiScalarMulShort(g1s, zs[:5], 64)
