"""Device-result MSM plans and handles on the GPU (include/mlhip.h, "device results"; include/mlhip_device_result.h, here through
the binding's functions of the same names): the tail of the MSM runs as a kernel (mathlib_amd/csrc/msm_tail.h) and the result
stays in device memory, in stream order, without a host wait.  The expected value everywhere is oracle.cref's MSM (over the
masked scalars for short plans) AND the bytes of a host-result plan of the same geometry in the same process.
Without the feature every test here fails where it creates its first plan or handle (MLHIP_EINVAL)."""
import ctypes
import time

import pytest

import stream_order_cases as S
import test_msm_bits_gpu as B
from conftest import load_golden
from test_stream_order_gpu import guarded  # a HIP error ends the module's GPU work: nothing more is started after one

pytestmark = pytest.mark.gpu

CURVES = B.CURVES
FR_BITS = B.FR_BITS


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(scope="module")
def delay(lib, mlhip):
    d = S.Delay(lib, mlhip)
    assert 50.0 <= d.ms <= 2000.0, (d.repeat, d.ms)
    return d


def dev(data):
    import torch

    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def slot(nbytes, fill=0xA5):
    import torch

    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def stream0():
    import torch

    return torch.cuda.current_stream().cuda_stream


def normalise(curve, group, xyzz):
    """(X / ZZ, Y / ZZZ) of an XYZZ value in Python integers, as affine Montgomery bytes; ZZ = 0 is the point at infinity"""
    from oracle import pyref as R

    cp = R.CURVES[curve]
    fb = cp.fp_bytes
    e = [R.fp_from_mont_bytes(cp, xyzz[i * fb : (i + 1) * fb]) for i in range(4 * group)]
    if group == 1:
        X, Y, ZZ, ZZZ = e
        if ZZ == 0:
            return bytes(2 * fb)
        return R.g1_to_mont_bytes(cp, (X * R.fp_inv(ZZ, cp.p) % cp.p, Y * R.fp_inv(ZZZ, cp.p) % cp.p))
    T = R.tower(cp)
    X, Y, ZZ, ZZZ = [T.f2(e[2 * i], e[2 * i + 1]) for i in range(4)]
    if T.f2_is_zero(ZZ):
        return bytes(4 * fb)
    return R.g2_to_mont_bytes(cp, (T.f2_mul(X, T.f2_inv(ZZ)), T.f2_mul(Y, T.f2_inv(ZZZ))))


class Pair:
    """a device-result plan and a host-result plan of the same geometry, with a device slot for [affine | XYZZ]"""

    def __init__(self, mlhip, cid, group, max_n, c, bits=0):
        self.dev = mlhip.MsmPlan(cid, group, max_n, c, bits, device_result=True)
        try:
            self.host = mlhip.MsmPlan(cid, group, max_n, c, bits)
        except BaseException:
            self.dev.close()
            raise
        self.psz = self.dev.point_bytes
        self.out = slot(3 * self.psz)

    def both(self, dp, ds, n, mont, st=None):
        """(affine, XYZZ) from the device-result plan after one synchronise, and the host-result plan's affine bytes"""
        import torch

        st = stream0() if st is None else st
        self.out.fill_(0xA5)
        self.dev.run_device(dp, ds, n, mont, st, self.out.data_ptr(), self.out.data_ptr() + self.psz)
        torch.cuda.synchronize()
        raw = host(self.out)
        return raw[: self.psz], raw[self.psz :], self.host.run(dp, ds, n, mont, st)

    def close(self):
        import torch

        torch.cuda.synchronize()
        self.dev.close()
        self.host.close()


GRID = [(c, 1) for c in CURVES] + [("BLS12-381", 2), ("BN254", 2)]
N_GRID = (5000, 257, 3, 2, 1)


@pytest.mark.parametrize("bits", [0, 33, 128])
@pytest.mark.parametrize("curve,group", GRID)
@guarded
def test_grid(lib, mlhip, curve, group, bits, monkeypatch):
    """every n of {1, 2, 3, 257, 5000} at c in {4, 8, 13, 16} on ONE plan of 5000 points (reused with every shorter n) and at
    c = 0 on a plan of its own size; plain scalars everywhere, Montgomery rows at c = 13; n = 5000 in five tiles, two tiles and
    one pass; the XYZZ value normalises to the affine point"""
    cid = load_golden(curve)["curve_id"]
    monkeypatch.delenv("MLHIP_TILE_LOG2", raising=False)
    data = {}
    for n in N_GRID:
        pts = B.points(curve, group, n)
        for mont in (False, True):
            sc, masked = B.scalars(curve, n, bits, mont)
            data[n, mont] = (dev(pts), dev(sc), B.oracle(cid, group, pts, masked, n))
    for c in (4, 8, 13, 16):
        pair = Pair(mlhip, cid, group, 5000, c, bits)
        try:
            assert pair.dev.is_device_result() and not pair.host.is_device_result()
            assert pair.dev.window() == pair.host.window() == B.windows(curve, bits, c)
            assert pair.dev.scalar_bits() == pair.host.scalar_bits() == B.eff_bits(curve, bits)
            for n in N_GRID:
                for mont in (False, True) if c == 13 else (False,):
                    dp, ds, want = data[n, mont]
                    for tile in ("10", "12", "0") if n == 5000 else ("0",):
                        monkeypatch.setenv("MLHIP_TILE_LOG2", tile)
                        aff, xyzz, host_aff = pair.both(dp.data_ptr(), ds.data_ptr(), n, mont)
                        assert aff == want == host_aff, (curve, group, bits, c, n, mont, tile)
                        assert normalise(curve, group, xyzz) == aff, (curve, group, bits, c, n)
        finally:
            pair.close()
    monkeypatch.delenv("MLHIP_TILE_LOG2", raising=False)
    for n in N_GRID:
        pair = Pair(mlhip, cid, group, n, 0, bits)
        try:
            dp, ds, want = data[n, False]
            aff, xyzz, host_aff = pair.both(dp.data_ptr(), ds.data_ptr(), n, False)
            assert aff == want == host_aff and normalise(curve, group, xyzz) == aff, (curve, group, bits, n)
        finally:
            pair.close()


def window_offsets(curve, c):
    """first bit of every window of a full-width plan at width c (msm_body.h: msm_win_layout)"""
    B1 = FR_BITS[curve] + 1
    W = -(-B1 // c)
    base, rem = B1 // W, B1 % W
    return [w * base + min(w, rem) for w in range(W)]


def sc_bytes(values):
    return b"".join((v % (1 << 256)).to_bytes(32, "little") for v in values)


@pytest.mark.parametrize("c", [8, 16])
@pytest.mark.parametrize("curve,group", [("BLS12-381", 1), ("BLS12-381", 2), ("BLS12-377", 1), ("BN254", 2)])
@guarded
def test_degenerate_tails(lib, mlhip, curve, group, c):
    """what the Horner pass of the tail kernel must survive: no pairs, all scalars 0, P beside -P, empty upper windows, r - 1
    and the unreduced 2^256 - 1, and the three hand cases -- a window sum EQUAL to the running value, OPPOSITE to it, and a
    cancellation in the middle of the pass after which it goes on"""
    from oracle import cref
    from oracle import pyref as R

    cp = R.CURVES[curve]
    cid = cp.curve_id
    psz = 2 * group * cp.fp_bytes
    base = B.points(curve, group, 16)  # (7 and 15 are infinities, 11 = -10)
    P, Rp = base[:psz], base[2 * psz : 3 * psz]
    offs = window_offsets(curve, c)
    k1, k2 = offs[1], offs[2]
    neg = lambda pt, k: cref.point_mul(cid, group, pt, (cp.r - (1 << k)) % cp.r)
    cases = {
        "all scalars zero": (base[: 5 * psz], [0] * 5),
        "P and -P": (base[10 * psz : 12 * psz] + Rp, [0xABCDEF123456789, 0xABCDEF123456789, 0]),
        "scalars below 2^16": (base[: 6 * psz], [1, 2, 65535, 32768, 40000, 77]),
        "r - 1 and 2^256 - 1": (base[: 3 * psz], [cp.r - 1, (1 << 256) - 1, cp.r - 1]),
        "equal operands": (P + cref.point_mul(cid, group, P, 1 << k1), [1 << k1, 1]),
        "opposite operands": (P + neg(P, k1), [1 << k1, 1]),
        "cancels mid-pass": (P + neg(P, k2 - k1) + Rp, [1 << k2, 1 << k1, 1]),
    }
    pair = Pair(mlhip, cid, group, 16, c)
    try:
        aff, xyzz, host_aff = pair.both(0, 0, 0, False)
        assert aff == bytes(psz) == host_aff and normalise(curve, group, xyzz) == bytes(psz), "n = 0"
        empty_xyzz = xyzz
        for tag, (pts, vals) in cases.items():
            n = len(vals)
            sc = sc_bytes(vals)
            want = cref.msm(cid, group, pts, sc, n, False, 0, 1)
            dp, ds = dev(pts), dev(sc)
            aff, xyzz, host_aff = pair.both(dp.data_ptr(), ds.data_ptr(), n, False)
            assert aff == want == host_aff, (curve, group, c, tag)
            assert normalise(curve, group, xyzz) == aff, (curve, group, c, tag)
            if tag in ("all scalars zero", "P and -P", "opposite operands"):
                assert aff == bytes(psz) and xyzz == empty_xyzz, tag  # the infinity form: (1, 1, 0, 0)
            if tag == "cancels mid-pass":
                assert aff == Rp
    finally:
        pair.close()


@pytest.mark.parametrize("flavours", ["dd", "dh", "hd"])
@guarded
def test_shared_launch(lib, mlhip, flavours, monkeypatch):
    """mlhip_msm_launch_shared with each plan of either flavour, each finished in its own way: equal widths (one sort, tiles) and
    unequal widths (one after the other)"""
    import torch

    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n = 3000
    p1, p2 = B.points(curve, 1, n), B.points(curve, 2, n)
    sc, masked = B.scalars(curve, n, 0, False)
    d1, d2, ds = dev(p1), dev(p2), dev(sc)
    want = [B.oracle(cid, 1, p1, masked, n), B.oracle(cid, 2, p2, masked, n)]
    out = slot(96 + 192)
    st = stream0()
    monkeypatch.setenv("MLHIP_TILE_LOG2", "10")
    for c1, c2 in ((13, 13), (13, 8)):
        plans = [mlhip.MsmPlan(cid, g, n, c, device_result=(f == "d")) for g, c, f in zip((1, 2), (c1, c2), flavours)]
        try:
            for m in (n, 1111):
                out.fill_(0xA5)
                plans[0].launch_shared(plans[1], d1.data_ptr(), d2.data_ptr(), ds.data_ptr(), m, False, st)
                got = []
                for g, p in enumerate(plans):
                    if p.is_device_result():
                        p.finish_device(out.data_ptr() + 96 * g)
                        got.append(None)
                    else:
                        got.append(p.finish())
                torch.cuda.synchronize()
                raw = host(out)
                got = [raw[:96] if got[0] is None else got[0], raw[96:] if got[1] is None else got[1]]
                if m == n:
                    assert got == want, (flavours, c1, c2)
                else:
                    assert got == [B.oracle(cid, 1, p1, masked, m), B.oracle(cid, 2, p2, masked, m)], (flavours, c1, c2, m)
        finally:
            torch.cuda.synchronize()
            for p in plans:
                p.close()


N_BASES = 1500


@pytest.mark.parametrize("window_c", [0, 16])
@pytest.mark.parametrize("tables", ["1", "0", "fold20"])
@pytest.mark.parametrize("curve,group", [("BLS12-381", 1), ("BLS12-381", 2), ("BLS12-377", 1)])
@guarded
def test_handles(lib, mlhip, curve, group, tables, window_c, monkeypatch):
    """a device-result handle beside a default handle on the same 1 500 points: mlhip_bases_msm_to_device into a device slot,
    with shifted-base tables (13-bit digits: one bucket group; MLHIP_FOLD_WINDOW=20: sixteen groups, combined on the device)
    and without; n = 0 and n below the count; mlhip_bases_msm is MLHIP_EINVAL; the batch call still works"""
    import torch

    cid = load_golden(curve)["curve_id"]
    monkeypatch.delenv("MLHIP_FOLD_WINDOW", raising=False)
    monkeypatch.setenv("MLHIP_BASES_TABLES", "0" if tables == "0" else "1")
    if tables == "fold20":
        monkeypatch.setenv("MLHIP_FOLD_WINDOW", "20")
    pts = B.points(curve, group, N_BASES)
    psz = len(pts) // N_BASES
    sc, masked = B.scalars(curve, N_BASES, 0, False)
    ds = dev(sc)
    h = mlhip.bases_create_device_result(cid, group, pts, N_BASES, window_c)
    ref = ctypes.c_void_p()
    try:
        mlhip.check(lib.mlhip_bases_create(cid, group, pts, N_BASES, window_c, ctypes.byref(ref)))
        assert mlhip.mlhip_msm_plan_is_device_result(lib, lib.mlhip_bases_plan(h)) == (0, 1)
        assert mlhip.mlhip_msm_plan_is_device_result(lib, lib.mlhip_bases_plan(ref)) == (0, 0)
        folded = mlhip.plan_timings(lib, lib.mlhip_bases_plan(h))["tables"]
        assert folded == mlhip.plan_timings(lib, lib.mlhip_bases_plan(ref))["tables"] == (0.0 if tables == "0" else 1.0)
        if curve == "BLS12-377":
            assert lib.mlhip_bases_checked_subgroup(h) == 1 == lib.mlhip_bases_checked_subgroup(ref)  # the Edwards path
        out = slot(psz)
        st = stream0()
        for n in (N_BASES, 0, 700, N_BASES):
            out.fill_(0xA5)
            mlhip.check(mlhip.mlhip_bases_msm_to_device(lib, h, ds.data_ptr() if n else None, 0, n, st, out.data_ptr()))
            torch.cuda.synchronize()
            ref_out = ctypes.create_string_buffer(psz)
            mlhip.check(lib.mlhip_bases_msm_device(ref, ds.data_ptr(), 0, n, st, ref_out))
            want = B.oracle(cid, group, pts, masked, n) if n else bytes(psz)
            assert host(out) == want == ref_out.raw, (curve, group, tables, window_c, n)
        # the host form has nowhere to put its result: MLHIP_EINVAL, nothing written
        o = ctypes.create_string_buffer(b"\x5a" * psz, psz)
        for n in (N_BASES, 0):
            assert lib.mlhip_bases_msm(h, sc, 0, n, o) == mlhip.EINVAL and b"mlhip_bases_msm_device" in lib.mlhip_last_error()
            assert o.raw == b"\x5a" * psz
        # ... and the default handle refuses the wrapper, which would treat a host pointer as a device one
        assert mlhip.mlhip_bases_msm_to_device(lib, ref, ds.data_ptr(), 0, N_BASES, st, out.data_ptr()) == mlhip.EINVAL
        lengths = [3, 0, 40]
        got = mlhip.bases_msm_batch(lib, h, psz, sc[: 43 * 32], False, lengths)
        want = mlhip.bases_msm_batch(lib, ref, psz, sc[: 43 * 32], False, lengths)
        assert got == want and got[1] == bytes(psz)
        assert got[0] == B.oracle(cid, group, pts, sc[: 3 * 32], 3)
    finally:
        torch.cuda.synchronize()
        lib.mlhip_bases_destroy(h)
        if ref:
            lib.mlhip_bases_destroy(ref)


@guarded
def test_flag_plumbing(lib, mlhip):
    """[12] of mlhip_msm_plan_timings is the flavour and appears only with cap >= 13; the five entry points that return their
    result in host memory or over a device list reject the flag with nothing written; what is left of a flagged window_c is
    checked as before"""
    import torch

    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n = B.N_HOST
    p1, p2 = B.points(curve, 1, n), B.points(curve, 2, n)
    sc, _ = B.scalars(curve, n, 0, False)
    FLAG = mlhip.WINDOW_DEVICE_RESULT
    for on in (False, True):
        plan = mlhip.MsmPlan(cid, 1, 1000, 13, device_result=on)
        try:
            for cap in (11, 12, 13, 20):
                buf = (ctypes.c_float * 20)(*([-7.0] * 20))
                k = lib.mlhip_msm_plan_timings(plan._h, buf, cap)
                assert k == min(cap, 13)
                assert all(buf[i] == -7.0 for i in range(k, 20))
                if k == 13:
                    assert buf[12] == (1.0 if on else 0.0) and buf[11] == FR_BITS[curve] and buf[7] == 13.0
            assert plan.is_device_result() is on
        finally:
            plan.close()
    dev0 = (ctypes.c_int * 1)(0)
    for wc in (FLAG, FLAG | 16, FLAG | mlhip.window_bits(16, 64)):
        o1, o2 = ctypes.create_string_buffer(b"\x5a" * 96, 96), ctypes.create_string_buffer(b"\x5a" * 192, 192)
        for m in (n, 0):
            assert lib.mlhip_msm_g1(cid, p1, sc, 0, m, wc, o1) == mlhip.EINVAL
            assert lib.mlhip_msm_g2(cid, p2, sc, 0, m, wc, o2) == mlhip.EINVAL
            assert lib.mlhip_msm_g1g2(cid, p1, p2, sc, 0, m, wc, o1, o2) == mlhip.EINVAL
            assert lib.mlhip_msm_multi(cid, 1, dev0, 1, p1, sc, 0, m, wc, o1) == mlhip.EINVAL
            assert lib.mlhip_msm_multi(cid, 2, dev0, 1, p2, sc, 0, m, wc, o2) == mlhip.EINVAL
        h = ctypes.c_void_p(1)
        assert lib.mlhip_bases_create_multi(cid, 1, dev0, 1, p1, n, wc, ctypes.byref(h)) == mlhip.EINVAL and not h.value
        assert o1.raw == b"\x5a" * 96 and o2.raw == b"\x5a" * 192
    # the flag comes off first; the rest is read as before
    dp = dev(p1)
    for wc in (FLAG | 21, FLAG | 3, FLAG | mlhip.window_bits(16, 257), FLAG | mlhip.window_bits(16, -1), FLAG | (300 << 8) | 16):
        h = ctypes.c_void_p(1)
        assert lib.mlhip_msm_plan_create(cid, 1, 1000, wc, ctypes.byref(h)) == mlhip.EINVAL and not h.value, wc
    for wc in (FLAG | 21, FLAG | mlhip.window_bits(16, 64)):  # the handles: a packed width is a width above 20
        h = ctypes.c_void_p(1)
        assert lib.mlhip_bases_create(cid, 1, p1, n, wc, ctypes.byref(h)) == mlhip.EINVAL and not h.value
        h = ctypes.c_void_p(1)
        assert lib.mlhip_bases_create_device(cid, 1, dp.data_ptr(), n, wc, ctypes.byref(h)) == mlhip.EINVAL and not h.value
    # the wrappers refuse a host-result plan (its outputs are host pointers)
    plan = mlhip.MsmPlan(cid, 1, 1000, 13)
    try:
        out = slot(96)
        assert mlhip.mlhip_msm_run_device(lib, plan._h, None, None, 0, 0, None, out.data_ptr(), None) == mlhip.EINVAL
        assert mlhip.mlhip_msm_finish_device(lib, plan._h, out.data_ptr(), None) == mlhip.EINVAL
        assert mlhip.mlhip_msm_plan_is_device_result(lib, None)[0] == mlhip.EINVAL
    finally:
        torch.cuda.synchronize()
        plan.close()


@guarded
def test_profiled_tail(lib, mlhip):
    """with profiling on, mlhip_msm_plan_timings waits for the plan's work and reports the tail kernel's time as [5]"""
    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n = 5000
    pts = B.points(curve, 1, n)
    sc, masked = B.scalars(curve, n, 0, False)
    dp, ds = dev(pts), dev(sc)
    out = slot(96)
    plan = mlhip.MsmPlan(cid, 1, n, 13, device_result=True)
    try:
        plan.set_profiling(True)
        plan.run_device(dp.data_ptr(), ds.data_ptr(), n, False, stream0(), out.data_ptr())
        t = plan.timings()  # (waits for `done`)
        assert host(out) == B.oracle(cid, 1, pts, masked, n)
        assert t["accumulate"] > 0 and t["device_total"] >= t["accumulate"] and 0 < t["host_tail"] < 50.0, t
    finally:
        plan.close()


# ---- busy stream (the scheme of tests/test_stream_order_gpu.py) ---------------------------------------------------------------


class DeviceMsm(S.Msm):
    """S.Msm on a device-result plan: the result is a device output, the call is asynchronous"""

    def __init__(self, cid, group, how, tile, **kw):
        super().__init__(cid, group, how, tile, **kw)
        self.out_bytes = [self.psz]
        self._out = None

    def open(self, lib, mlhip):
        self.h = ctypes.c_void_p()
        mlhip.check(mlhip.mlhip_msm_plan_create_device_result(lib, self.cid, self.group, self.n, self.c, 0, ctypes.byref(self.h)))

    def call(self, lib, mlhip, ins, outs, host, stream):
        if self.how == "run":
            mlhip.check(mlhip.mlhip_msm_run_device(lib, self.h, ins[0], ins[1], 0, self.n, stream, outs[0], None))
        else:
            mlhip.check(lib.mlhip_msm_launch(self.h, ins[0], ins[1], 0, self.n, stream))
            mlhip.check(mlhip.mlhip_msm_finish_device(lib, self.h, outs[0], None))
        return []

    def finish(self, lib, mlhip):
        return []


class DeviceBasesMsm(S.BasesMsm):
    """mlhip_bases_msm_to_device on a device-result handle"""

    def __init__(self, cid, group=1, n=3000):
        super().__init__(cid, group, n)
        self.out_bytes = [self.psz]

    def open(self, lib, mlhip):
        self.h = mlhip.bases_create_device_result(self.cid, self.group, self.bases, self.n, 0)

    def close(self, lib):
        if self.h:
            lib.mlhip_bases_destroy(self.h)
            self.h = None

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(mlhip.mlhip_bases_msm_to_device(lib, self.h, ins[0], 0, self.n, stream, outs[0]))
        return []

    def host_form(self, lib, mlhip, ins, host):
        return None


BUSY = {
    "run_device-g1-tiles": lambda: DeviceMsm(1, 1, "run", 10),
    "run_device-g2-one-pass": lambda: DeviceMsm(0, 2, "run", 0),
    "launch+finish_device-g1": lambda: DeviceMsm(2, 1, "launch", 10),
    "bases_msm_to_device-g1": lambda: DeviceBasesMsm(1, 1),
    "bases_msm_to_device-g2": lambda: DeviceBasesMsm(2, 2),
}


@pytest.mark.parametrize("tag", sorted(BUSY))
@guarded
def test_busy_stream(lib, mlhip, delay, tag, monkeypatch):
    """inputs still being produced in front of the call, the call returns while the stream is busy (asserted), inputs and the
    output slot overwritten right behind it: run_scenario of tests/stream_order_cases.py with sync = None"""
    import torch

    case = BUSY[tag]()
    for name in ("MLHIP_TILE_LOG2", "MLHIP_BASES_TABLES", "MLHIP_FOLD_WINDOW"):
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    log = []
    outcome = S.run_scenario(lib, mlhip, case, torch.cuda.Stream(), delay, log.append, tag, None)
    assert outcome.busy and outcome.call_ms < delay.ms / 2


@guarded
def test_two_runs_on_two_streams(lib, mlhip, delay, monkeypatch):
    """two consecutive runs of ONE plan on two different streams: the first waits behind the delay on s1, the second is queued
    on the idle s2 at once -- it must wait for the first on the device (the plan's buffers and slot are shared), and neither
    call waits on the host"""
    import torch

    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n = 3000
    monkeypatch.setenv("MLHIP_TILE_LOG2", "10")
    pa = pb = B.points(curve, 1, n)  # one point array, two scalar vectors
    sa, ma = B.scalars(curve, n, 0, False, seed=1)
    sb, mb_ = B.scalars(curve, n, 0, False, seed=2)
    want_a, want_b = B.oracle(cid, 1, pa, ma, n), B.oracle(cid, 1, pb, mb_, n)
    assert want_a != want_b
    dpa, dsa, dsb = dev(pa), dev(sa), dev(sb)
    out = slot(2 * 96)
    plan = mlhip.MsmPlan(cid, 1, n, 13, device_result=True)
    s1 = torch.cuda.Stream()
    try:
        plan.run_device(dpa.data_ptr(), dsa.data_ptr(), n, False, s1.cuda_stream, out.data_ptr())  # warm-up
        s1.synchronize()
        assert host(out)[:96] == want_a
        s2 = delay.independent_stream(s1)
        out.fill_(0xA5)
        delay.clear()
        delay.queue(s1)
        t0 = time.perf_counter()
        plan.run_device(dpa.data_ptr(), dsa.data_ptr(), n, False, s1.cuda_stream, out.data_ptr())
        plan.run_device(dpa.data_ptr(), dsb.data_ptr(), n, False, s2.cuda_stream, out.data_ptr() + 96)
        call_ms = 1e3 * (time.perf_counter() - t0)
        busy = not s1.query()
        s2.synchronize()  # (s2 waited for the first run's `done`, behind the delay on s1)
        s1.synchronize()
        delay.check()
        raw = host(out)
        assert raw[:96] == want_a and raw[96:] == want_b
        assert busy and call_ms < delay.ms / 2, (busy, call_ms, delay.ms)
    finally:
        torch.cuda.synchronize()
        plan.close()


@guarded
def test_chain_into_pairing(lib, mlhip):
    """a batch verifier's chain: two 128-bit device-result MSMs of 257 points write slots 0 and 1 of a G1 array that
    mlhip_pairing_prepared_device reads at ppp = 2 on the same stream, with no host wait in between and one synchronise at
    the end; the expected value is the host route (host-result plans, then mlhip_pairing_prepared)"""
    import torch

    curve = "BLS12-381"
    cid = load_golden(curve)["curve_id"]
    n, bits = 257, 128
    pa, pb = B.points(curve, 1, n), B.points(curve, 1, 300)[43 * 96 :]
    sa, _ = B.scalars(curve, n, bits, False, seed=3)
    sb, _ = B.scalars(curve, n, bits, False, seed=4)
    qs = S._pts(cid, 2, 15, 2)
    dpa, dpb, dsa, dsb = dev(pa), dev(pb), dev(sa), dev(sb)
    d_g1, d_gt = slot(2 * 96), slot(576)
    st = torch.cuda.Stream()
    hq = ctypes.c_void_p()
    mlhip.check(lib.mlhip_g2_prepared_create(cid, qs, 2, ctypes.byref(hq)))
    plans = [mlhip.MsmPlan(cid, 1, n, 0, bits, device_result=True) for _ in range(2)]
    hosts = [mlhip.MsmPlan(cid, 1, n, 0, bits) for _ in range(2)]
    try:
        torch.cuda.synchronize()
        plans[0].run_device(dpa.data_ptr(), dsa.data_ptr(), n, False, st.cuda_stream, d_g1.data_ptr())
        plans[1].run_device(dpb.data_ptr(), dsb.data_ptr(), n, False, st.cuda_stream, d_g1.data_ptr() + 96)
        mlhip.check(lib.mlhip_pairing_prepared_device(hq, d_g1.data_ptr(), None, 2, 1, d_gt.data_ptr(), st.cuda_stream))
        st.synchronize()
        a = hosts[0].run(dpa.data_ptr(), dsa.data_ptr(), n, False, st.cuda_stream)
        b = hosts[1].run(dpb.data_ptr(), dsb.data_ptr(), n, False, st.cuda_stream)
        assert host(d_g1) == a + b and a != bytes(96) != b
        want = ctypes.create_string_buffer(576)
        mlhip.check(lib.mlhip_pairing_prepared(hq, a + b, None, 2, 1, want))
        assert host(d_gt) == want.raw
    finally:
        torch.cuda.synchronize()
        for p in plans + hosts:
            p.close()
        lib.mlhip_g2_prepared_destroy(hq)


@guarded
def test_batch_of_results(lib, mlhip):
    """16 runs of one plan, each with another n, into a 16-slot device array: one synchronise, one copy, 16 values"""
    import torch

    curve = "BN254"
    cid = load_golden(curve)["curve_id"]
    nmax = 2000
    pts = B.points(curve, 1, nmax)
    sc, masked = B.scalars(curve, nmax, 0, False)
    dp, ds = dev(pts), dev(sc)
    psz = len(pts) // nmax
    out = slot(16 * psz)
    ns = [nmax - 117 * k for k in range(15)] + [0]
    plan = mlhip.MsmPlan(cid, 1, nmax, 13, device_result=True)
    try:
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        for k, n in enumerate(ns):
            plan.run_device(dp.data_ptr(), ds.data_ptr(), n, False, st.cuda_stream, out.data_ptr() + k * psz)
        st.synchronize()
        raw = host(out)
        for k, n in enumerate(ns):
            want = B.oracle(cid, 1, pts, masked, n) if n else bytes(psz)
            assert raw[k * psz : (k + 1) * psz] == want, (k, n)
    finally:
        torch.cuda.synchronize()
        plan.close()
