"""Sets of resident-bases handles on the GPU (include/mlhip.h, "sets of handles"; include/mlhip_bases_set.h): the MSMs of up
to four tables over ONE scalar vector from one upload and one sort train per geometry class.  Expected bytes come from the C
oracle per member (computed once per (curve, member, scalars, prefix) and shared), and from each member's own mlhip_bases_msm.

Every member has 300 bases (the smallest size at which the paths differ: tiles of 64 give five tiles with a ragged last one,
a digit width of 17 gives two bucket groups), its own point set and a base at infinity.  The scalars hold 0, 1, r - 1 and an
unreduced value >= r; both scalars_mont forms; the all-equal vector puts every digit of every scalar into one bucket, so the
long-bucket slices of every member gather through another plan's lists."""
import ctypes
import functools
import threading

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
N = 300
PREFIXES = (0, 1, 63, 64, 65, 300)
SWITCHES = ("MLHIP_BASES_TABLES", "MLHIP_FOLD_WINDOW", "MLHIP_FOLD_TILE_LOG2", "MLHIP_STREAM_SEGMENTS", "MLHIP_STREAM_SCHEDULE",
            "MLHIP_TILE_LOG2", "MLHIP_SORT_AHEAD", "MLHIP_BASES_SET_SHARE", "MLHIP_EDWARDS")


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    """every test starts from the library's defaults, with the shared route forced: the tiny sizes here are below any size the
    default dispatch may leave to the per-member route (mathlib_amd/csrc/msm_set.h: MLHIP_SET_SHARE_MIN_N_HOST / _DEVICE)"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MLHIP_BASES_SET_SHARE", "1")


def _cid(curve):
    return load_golden(curve)["curve_id"]


def _r(curve):
    from oracle import pyref as R

    return R.CURVES[curve].r


@functools.lru_cache(maxsize=None)
def points(cid, group, seed, n=N):
    """n distinct points of the subgroup, the 18th replaced by the point at infinity"""
    from oracle import cref

    psz = len(cref.gen_points(cid, group, 1, 1, 1))
    pts = bytearray(cref.gen_points(cid, group, 900 + 31 * seed + group, 5 + 2 * seed, n))
    pts[17 * psz : 18 * psz] = bytes(psz)
    return bytes(pts)


def _limbs(v):
    return [(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]


@functools.lru_cache(maxsize=None)
def scalars(curve, kind):
    """(bytes of N scalars, scalars_mont).  "mixed": random 256-bit values with 0, 1, r - 1 and an unreduced value >= r;
    "mont": values below r read as Montgomery residues, with 0 and r - 1; "same": the all-equal vector"""
    r = _r(curve)
    rng = np.random.default_rng(4000 + CURVES.index(curve))
    if kind == "same":
        return np.tile(np.array([_limbs(int.from_bytes(b"\x01" * 32, "little"))], dtype=np.uint64), (N, 1)).tobytes(), 0
    sc = rng.integers(0, 1 << 64, size=(N, 4), dtype=np.uint64, endpoint=False)
    if kind == "mont":
        sc[:, 3] >>= np.uint64(4)  # below 2^252 < r on all three curves
        for i, v in ((0, 0), (1, r - 1), (64, 1)):
            sc[i] = _limbs(v)
        return sc.tobytes(), 1
    for i, v in ((0, 0), (1, 1), (2, r - 1), (3, r + 5), (63, (1 << 256) - 1), (64, r - 1), (299, r)):
        sc[i] = _limbs(v)
    return sc.tobytes(), 0


@functools.lru_cache(maxsize=None)
def want(curve, group, seed, kind, n, n_bases=N):
    from oracle import cref

    if n == 0:
        return bytes(len(points(_cid(curve), group, seed, n_bases)) // n_bases)
    sc, mont = scalars(curve, kind)
    return cref.msm(_cid(curve), group, points(_cid(curve), group, seed, n_bases), sc, n, bool(mont), 0, 8)


class Members:
    """handles over their own point sets (member i: seed i), and a set over them"""

    def __init__(self, lib, mlhip, curve, groups, window_c=None, n_bases=None):
        self.lib, self.mlhip, self.curve, self.cid = lib, mlhip, curve, _cid(curve)
        self.groups = list(groups)
        self.n_bases = list(n_bases or [N] * len(self.groups))
        self.psz = [mlhip.sizes(self.cid)[g] for g in self.groups]
        self.h = []
        self.set = None
        try:
            for i, g in enumerate(self.groups):
                h = ctypes.c_void_p()
                wc = window_c[i] if window_c else 0
                mlhip.check(lib.mlhip_bases_create(self.cid, g, points(self.cid, g, i, self.n_bases[i]), self.n_bases[i], wc, ctypes.byref(h)))
                self.h.append(h)
            self.set = mlhip.bases_set_create(lib, self.h)
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        if self.set:
            self.lib.mlhip_bases_destroy(self.set)
            self.set = None
        for h in self.h:
            self.lib.mlhip_bases_destroy(h)
        self.h = []

    def tables(self):
        return [self.mlhip.plan_timings(self.lib, self.lib.mlhip_bases_plan(h)).get("tables") == 1.0 for h in self.h]

    def expected(self, kind, n):
        return [want(self.curve, g, i, kind, n, self.n_bases[i]) for i, g in enumerate(self.groups)]

    def own(self, i, kind, n):
        sc, mont = scalars(self.curve, kind)
        out = ctypes.create_string_buffer(self.psz[i])
        self.mlhip.check(self.lib.mlhip_bases_msm(self.h[i], sc, mont, n, out))
        return out.raw

    def run(self, kind, n, device=False):
        """the set's MSM over the first n scalars: one result (bytes) per member"""
        sc, mont = scalars(self.curve, kind)
        out = ctypes.create_string_buffer(b"\xA5" * sum(self.psz), sum(self.psz))
        if device:
            import torch

            d = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to("cuda")
            self.mlhip.check(self.lib.mlhip_bases_msm_device(self.set, d.data_ptr(), mont, n, torch.cuda.current_stream().cuda_stream, out))
        else:
            self.mlhip.check(self.lib.mlhip_bases_msm(self.set, sc, mont, n, out))
        raw, res, off = out.raw, [], 0
        for sz in self.psz:
            res.append(raw[off : off + sz])
            off += sz
        return res

    def route(self):
        return self.mlhip.bases_set_route(self.lib, self.set)

    def check(self, kind, n, device=False, route=None, tag=""):
        got = self.run(kind, n, device)
        exp = self.expected(kind, n)
        for i in range(len(got)):
            assert got[i] == exp[i], (self.curve, self.groups, tag, kind, n, "device" if device else "host", "member %d" % i)
        if route is not None:
            assert self.route() == route, (self.curve, self.groups, tag, kind, n, "device" if device else "host")


@pytest.mark.parametrize("geometry", [(8, 20), (8, 6), (17, 6)], ids=["one-tile", "five-tiles", "two-groups"])
@pytest.mark.parametrize("groups", [(1, 1, 2), (2, 1)], ids=["g1-g1-g2", "g2-g1"])
@pytest.mark.parametrize("curve", CURVES)
def test_folded_one_class(lib, mlhip, curve, groups, geometry, monkeypatch):
    """members with shifted-base tables of one geometry: one sort train per tile and one upload for the whole set.  One tile; five
    tiles with a ragged last one (device scalars: sort-ahead into the helper records); two bucket groups."""
    c, tile_lg = geometry
    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", str(c))
    monkeypatch.setenv("MLHIP_FOLD_TILE_LOG2", str(tile_lg))
    k = len(groups)
    with Members(lib, mlhip, curve, groups) as m:
        assert m.tables() == [True] * k
        assert lib.mlhip_bases_plan(m.set) is None
        for n in PREFIXES:
            m.check("mixed", n, route=(k, 1 if n else 0, 1 if n else 0, 1), tag=geometry)
            m.check("mixed", n, device=True, route=(k, 1 if n else 0, 0, 1), tag=geometry)
        for kind in ("mont", "same"):
            m.check(kind, N, route=(k, 1, 1, 1), tag=geometry)
            m.check(kind, N, device=True, route=(k, 1, 0, 1), tag=geometry)
            m.check(kind, 65, device=True, tag=geometry)
        # each member's own MSM gives the same bytes, and the set still does after it
        for i in range(k):
            assert m.own(i, "mixed", N) == m.expected("mixed", N)[i]
        m.check("same", N, tag=geometry)
        # the sort of tile s + 1 in line instead of ahead: same bytes
        monkeypatch.setenv("MLHIP_SORT_AHEAD", "0")
        m.check("mixed", N, device=True, route=(k, 1, 0, 1), tag=(geometry, "sort in line"))
        m.check("same", N, device=True, tag=(geometry, "sort in line"))
        monkeypatch.delenv("MLHIP_SORT_AHEAD")
        # host scalars streamed in five equal segments, cut again at the tile boundaries: same bytes, still one upload
        monkeypatch.setenv("MLHIP_STREAM_SEGMENTS", "5")
        for kind in ("mixed", "same"):
            m.check(kind, N, route=(k, 1, 1, 1), tag=(geometry, "five segments"))
        m.check("mixed", 65, tag=(geometry, "five segments"))


@pytest.mark.parametrize("curve", CURVES)
def test_plain_one_class(lib, mlhip, curve):
    """both members on plain tables with window_c = 12: one class, as the shared-scalar pair of two plans"""
    with Members(lib, mlhip, curve, (1, 2), window_c=(12, 12)) as m:
        assert m.tables() == [False, False]
        for n in PREFIXES:
            m.check("mixed", n, route=(2, 1 if n else 0, 1 if n else 0, 0))
        for kind in ("mixed", "mont", "same"):
            m.check(kind, N, device=True, route=(2, 1, 0, 0))
        m.check("same", N, route=(2, 1, 1, 0))


@pytest.mark.parametrize("curve", CURVES)
def test_two_classes_one_upload(lib, mlhip, curve):
    """window_c 12 beside 13: two classes, and the scalars still cross once -- whether the class that uploads them is a train
    (two members) or a single member, and whichever comes first"""
    with Members(lib, mlhip, curve, (1, 2), window_c=(12, 13)) as m:
        for kind in ("mixed", "same"):
            m.check(kind, N, route=(2, 2, 1, 0))
            m.check(kind, N, device=True, route=(2, 2, 0, 0))
        m.check("mixed", 65, route=(2, 2, 1, 0))
    for wcs in ((12, 13, 12), (13, 12, 12)):
        with Members(lib, mlhip, curve, (1, 2, 2), window_c=wcs) as m:
            for kind in ("mixed", "same"):
                m.check(kind, N, route=(3, 2, 1, 0), tag=wcs)
                m.check(kind, 64, route=(3, 2, 1, 0), tag=wcs)
            m.check("mixed", N, device=True, route=(3, 2, 0, 0), tag=wcs)


@pytest.mark.parametrize("curve", CURVES)
def test_default_policy_folded_g1_beside_plain_g2(lib, mlhip, curve):
    """the library's own geometry: 1100 G1 bases get shifted-base tables, 300 G2 bases stay plain -- two classes, one upload"""
    with Members(lib, mlhip, curve, (1, 2), n_bases=(1100, N)) as m:
        assert m.tables() == [True, False]
        for n in (N, 65):
            m.check("mixed", n, route=(2, 2, 1, 0))
            m.check("mixed", n, device=True, route=(2, 2, 0, 0))
        m.check("same", N, route=(2, 2, 1, 0))


def test_bls12_377_checked_g1_on_the_edwards_path_beside_g2(lib, mlhip, monkeypatch):
    """a subgroup-checked BLS12-377 G1 table sums its buckets in twisted Edwards coordinates from Niels rows; the G2 member of
    the same class gathers Weierstrass rows through the same lists"""
    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", "17")
    monkeypatch.setenv("MLHIP_FOLD_TILE_LOG2", "7")
    with Members(lib, mlhip, "BLS12-377", (1, 2, 1)) as m:
        assert [lib.mlhip_bases_checked_subgroup(h) for h in m.h] == [1, 0, 1]
        assert lib.mlhip_bases_checked_subgroup(m.set) == 0  # (1 iff every member's is)
        assert mlhip.plan_timings(lib, lib.mlhip_bases_plan(m.h[0])).get("tables") == 1.0
        for kind in ("mixed", "mont", "same"):
            m.check(kind, N, route=(3, 1, 1, 1))
            m.check(kind, N, device=True, route=(3, 1, 0, 1))
        m.check("mixed", 129, device=True)
        pair = mlhip.bases_set_create(lib, [m.h[0], m.h[2]])
        try:
            assert lib.mlhip_bases_checked_subgroup(pair) == 1
        finally:
            lib.mlhip_bases_destroy(pair)


@pytest.mark.parametrize("tables", ["1", "0"], ids=["tables", "plain"])
@pytest.mark.parametrize("curve", CURVES)
def test_share_off_runs_every_member_on_its_own(lib, mlhip, curve, tables, monkeypatch):
    """MLHIP_BASES_SET_SHARE=0: the second implementation -- the same bytes, k sorts and k uploads"""
    monkeypatch.setenv("MLHIP_BASES_TABLES", tables)
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", "8")
    monkeypatch.setenv("MLHIP_FOLD_TILE_LOG2", "6")
    t = 1 if tables == "1" else 0
    with Members(lib, mlhip, curve, (1, 1, 2), window_c=None if t else (12, 12, 12)) as m:
        assert m.tables() == [bool(t)] * 3
        monkeypatch.setenv("MLHIP_BASES_SET_SHARE", "0")
        for n in (N, 65, 0):
            m.check("mixed", n, route=(3, 3 if n else 0, 3 if n else 0, t))
            m.check("mixed", n, device=True, route=(3, 3 if n else 0, 0, t))
        m.check("same", N, route=(3, 3, 3, t))
        monkeypatch.setenv("MLHIP_BASES_SET_SHARE", "1")
        m.check("same", N, route=(3, 1, 1, t))


def test_members_stay_usable_on_their_own(lib, mlhip, monkeypatch):
    """a member's own MSM before, between and after set calls; destroying the set leaves the members working"""
    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", "8")
    monkeypatch.setenv("MLHIP_FOLD_TILE_LOG2", "6")
    curve = "BLS12-381"
    with Members(lib, mlhip, curve, (1, 2)) as m:
        exp = m.expected("mixed", N)
        assert m.own(0, "mixed", N) == exp[0]
        m.check("mixed", N)
        assert m.own(1, "mixed", N) == exp[1] and m.own(0, "mixed", 65) == m.expected("mixed", 65)[0]
        m.check("same", N, device=True)
        assert m.own(0, "same", N) == m.expected("same", N)[0]
        m.check("mixed", N, route=(2, 1, 1, 1))
        second = mlhip.bases_set_create(lib, [m.h[1], m.h[0]])  # the same members in a second set, the other way round
        out = mlhip.bases_set_msm(lib, second, [m.psz[1], m.psz[0]], scalars(curve, "mixed")[0], False, N)
        assert out == [exp[1], exp[0]]
        lib.mlhip_bases_destroy(second)
        lib.mlhip_bases_destroy(m.set)
        m.set = None
        assert m.own(0, "mixed", N) == exp[0] and m.own(1, "mixed", N) == exp[1]


def test_refusals(lib, mlhip, monkeypatch):
    cid = _cid("BLS12-381")
    EINVAL = mlhip.EINVAL

    def refused(handles, text):
        arr = (ctypes.c_void_p * 5)(*[h.value if isinstance(h, ctypes.c_void_p) else h for h in handles])
        s = ctypes.c_void_p(1)
        assert mlhip.mlhip_bases_set_create(lib, arr, len(handles), ctypes.byref(s)) == EINVAL and not s.value, text
        assert text in lib.mlhip_last_error().decode(), (text, lib.mlhip_last_error())

    with Members(lib, mlhip, "BLS12-381", (1, 2), window_c=(12, 13), n_bases=(N, 200)) as m, Members(lib, mlhip, "BN254", (1,)) as other:
        a, b = m.h
        refused([], "1 .. 4 members")
        refused([a, b, a, b, a], "1 .. 4 members")
        refused([a, None], "null member")
        refused([a, b, a], "listed twice")
        refused([a, m.set], "a set cannot be a member")
        refused([a, other.h[0]], "different curves")
        sharded = ctypes.c_void_p()
        devs = (ctypes.c_int * 2)(0, 0)
        mlhip.check(lib.mlhip_bases_create_multi(cid, 1, devs, 2, points(cid, 1, 0), N, 0, ctypes.byref(sharded)))
        dres = mlhip.bases_create_device_result(cid, 1, points(cid, 1, 0), N)
        try:
            refused([a, sharded], "spread over several devices")
            refused([dres, b], "device-result")
        finally:
            lib.mlhip_bases_destroy(sharded)
            lib.mlhip_bases_destroy(dres)
        # n above the smallest member's count
        sc, mont = scalars("BLS12-381", "mixed")
        out = ctypes.create_string_buffer(sum(m.psz))
        assert lib.mlhip_bases_msm(m.set, sc, mont, 201, out) == EINVAL and "smallest member" in lib.mlhip_last_error().decode()
        assert lib.mlhip_bases_msm_device(m.set, None, mont, 201, None, out) == EINVAL
        assert lib.mlhip_bases_msm(m.set, None, mont, 200, out) == EINVAL
        m.check("mixed", 200, route=(2, 2, 1, 0))
        # what a set is not
        assert lib.mlhip_bases_plan(m.set) is None
        tabled = ctypes.c_size_t()
        assert lib.mlhip_bases_batch_tabled(m.set, ctypes.byref(tabled)) == EINVAL and "set of handles" in lib.mlhip_last_error().decode()
        offs = (ctypes.c_uint64 * 2)(0, 1)
        assert lib.mlhip_bases_msm_batch(m.set, sc, mont, None, offs, 1, out) == EINVAL and "set of handles" in lib.mlhip_last_error().decode()
        assert lib.mlhip_bases_msm_batch_device(m.set, None, mont, None, offs, 1, None, None) == EINVAL
        assert "set of handles" in lib.mlhip_last_error().decode()
        # the route of a handle that is not a set
        info = (ctypes.c_int * 4)()
        assert mlhip.mlhip_bases_set_route(lib, a, info, 4) == EINVAL and "not a set" in lib.mlhip_last_error().decode()
        assert mlhip.mlhip_bases_set_route(lib, m.set, info, 2) == 2 and list(info) == [2, 2, 0, 0]


def test_two_threads_on_the_set_and_on_a_member(lib, mlhip, monkeypatch):
    """one thread on the set, one on a member, a handful of calls each: the set call holds every member's mutex"""
    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", "8")
    monkeypatch.setenv("MLHIP_FOLD_TILE_LOG2", "6")
    with Members(lib, mlhip, "BN254", (1, 2)) as m:
        exp = {kind: m.expected(kind, N) for kind in ("mixed", "same")}
        bad = []

        def on_set():
            try:
                for i in range(6):
                    kind = ("mixed", "same")[i & 1]
                    if m.run(kind, N) != exp[kind]:
                        bad.append(("set", i))
            except BaseException as e:  # noqa: BLE001
                bad.append(("set", repr(e)))

        def on_member():
            try:
                for i in range(6):
                    kind = ("same", "mixed")[i & 1]
                    if m.own(1, kind, N) != exp[kind][1]:
                        bad.append(("member", i))
            except BaseException as e:  # noqa: BLE001
                bad.append(("member", repr(e)))

        ts = [threading.Thread(target=on_set), threading.Thread(target=on_member)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not bad, bad


def test_device_form_on_a_busy_stream(lib, mlhip, monkeypatch):
    """mlhip_bases_msm_device on a set through the busy-stream scenario of tests/test_stream_order_gpu.py: the scalars are still
    being produced on the stream when the call is made, and are overwritten right behind it; synchronous by contract"""
    import torch

    import stream_order_cases as S

    class SetMsm(S.BasesMsm):
        """two members (G1, G2) with shifted-base tables in five tiles: the sort-ahead stream must wait for the producer too"""

        def __init__(self, cid, n=N):
            S.BasesMsm.__init__(self, cid, 1, n)
            self.member_bases = [S._pts(cid, 1, 14, n), S._pts(cid, 2, 15, n)]
            self.psz = [2 * S.FPB[cid], 4 * S.FPB[cid]]
            self.hs = []

        def open(self, lib, mlhip):
            for g, pts in zip((1, 2), self.member_bases):
                h = ctypes.c_void_p()
                mlhip.check(lib.mlhip_bases_create(self.cid, g, pts, self.n, 0, ctypes.byref(h)))
                self.hs.append(h)
            self.h = mlhip.bases_set_create(lib, self.hs)

        def close(self, lib):
            if self.h:
                lib.mlhip_bases_destroy(self.h)
                self.h = None
            for h in self.hs:
                lib.mlhip_bases_destroy(h)
            self.hs = []

        def call(self, lib, mlhip, ins, outs, host, stream):
            out = ctypes.create_string_buffer(sum(self.psz))
            mlhip.check(lib.mlhip_bases_msm_device(self.h, ins[0], 0, self.n, stream, out))
            assert mlhip.bases_set_route(lib, self.h) == (2, 1, 0, 1)
            return [out.raw]

        def host_form(self, lib, mlhip, ins, host):
            out = ctypes.create_string_buffer(sum(self.psz))
            mlhip.check(lib.mlhip_bases_msm(self.h, ins[0], 0, self.n, out))
            return [out.raw]

        def oracle(self, ins, host):
            return [b"".join(S._cref().msm(self.cid, g, pts, ins[0], self.n, False, 0, 8) for g, pts in zip((1, 2), self.member_bases))]

    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    monkeypatch.setenv("MLHIP_FOLD_WINDOW", "8")
    monkeypatch.setenv("MLHIP_FOLD_TILE_LOG2", "6")
    delay = S.Delay(lib, mlhip)
    assert 50.0 <= delay.ms <= 2000.0, (delay.repeat, delay.ms)
    log = []
    S.run_scenario(lib, mlhip, SetMsm(1), torch.cuda.Stream(), delay, log.append, "bases-set-msm", S.BASES_SYNC)


def test_python_mirror(lib, mlhip, monkeypatch):
    """mathlib_amd/driver.py: NewBasesSet(...).MultiScalarMul(scalars) returns one point per member"""
    from mathlib_amd import driver

    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    c = driver.NewCurve("BLS12_381")
    rng = np.random.default_rng(11)
    n = 40
    g1 = [c.GenG1().Mul(c.NewZrFromInt(int(v))) for v in rng.integers(1, 1 << 40, size=n)]
    g2 = [c.GenG2().Mul(c.NewZrFromInt(int(v))) for v in rng.integers(1, 1 << 40, size=n)]
    zs = [c.NewZrFromInt(int(v)) for v in rng.integers(0, 1 << 62, size=n)]
    a, b2 = c.NewBases(g1), c.NewBasesG2(g2)
    s = c.NewBasesSet(a, b2)
    try:
        got = s.MultiScalarMul(zs)
        assert len(got) == 2 and got[0].Equals(c.MultiScalarMul(g1, zs)) and got[1].Equals(c.MultiScalarMulG2(g2, zs))
        assert got[0].Equals(a.MultiScalarMul(zs)) and got[1].Equals(b2.MultiScalarMul(zs))
        assert s.Route() == (2, 1, 1, 1)
        few = s.MultiScalarMul(zs[:7])
        assert few[0].Equals(c.MultiScalarMul(g1[:7], zs[:7])) and few[1].Equals(c.MultiScalarMulG2(g2[:7], zs[:7]))
        with pytest.raises(IndexError):
            s.MultiScalarMul(zs + zs)
    finally:
        s.Close()
        a.Close()
        b2.Close()


def test_default_dispatch_follows_the_measured_thresholds(lib, mlhip, monkeypatch):
    """MLHIP_BASES_SET_SHARE unset: host scalars share from 2^12 on, device scalars from 2^16 on (mathlib_amd/csrc/msm_set.h);
    below, every member runs its own MSM.  Same bytes either way."""
    monkeypatch.delenv("MLHIP_BASES_SET_SHARE")
    monkeypatch.setenv("MLHIP_BASES_TABLES", "1")
    n = 1 << 12
    with Members(lib, mlhip, "BN254", (1, 2), n_bases=(n, n)) as m:
        sc = np.random.default_rng(5).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False).tobytes()
        own = []
        for h, sz in zip(m.h, m.psz):
            out = ctypes.create_string_buffer(sz)
            mlhip.check(lib.mlhip_bases_msm(h, sc, 0, n, out))
            own.append(out.raw)
        from oracle import cref

        assert own[0] == cref.msm(m.cid, 1, points(m.cid, 1, 0, n), sc, n, False, 0, 8)
        assert mlhip.bases_set_msm(lib, m.set, m.psz, sc, False, n) == own and m.route() == (2, 1, 1, 1)
        assert mlhip.bases_set_msm(lib, m.set, m.psz, sc, False, n - 1) != own and m.route() == (2, 2, 2, 1)
        import torch

        d = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to("cuda")
        out = ctypes.create_string_buffer(sum(m.psz))
        mlhip.check(lib.mlhip_bases_msm_device(m.set, d.data_ptr(), 0, n, torch.cuda.current_stream().cuda_stream, out))
        assert out.raw == b"".join(own) and m.route() == (2, 2, 0, 1)
