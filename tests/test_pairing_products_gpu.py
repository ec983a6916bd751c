"""K products of m > 4 pairs each in one call (include/mlhip.h: "products of any length", MLHIP_PRODUCT_PAIRS), on the GPU,
all three curves.

The expected value of a case is cref.final_exp(cref.miller_loop(cid, g1, g2, m, K, 8), K, 8): the oracle takes any m.  It is
computed once per (curve, case) and shared by every switch setting.  Raw Miller values are compared after mlhip_final_exp, as
the existing pairing tests do; among the library's own paths they are compared as bytes.

The cases are the smallest shapes at which the grouping, the tail, the fold and a block boundary can go wrong:
  k1m5    K = 1,  m = 5    4 + 1 tail
  k3m8    K = 3,  m = 8    exact groups, one fold pass at per = 4
  k13m17  K = 13, m = 17   65 groups at per = 4 (more than one 64-lane block in every shape), tail of 1, odd fold 5 -> 3 -> 2 -> 1
  inf     K = 2,  m = 9    G1 at infinity in pair 0, G2 at infinity in pair 5, pairs 4 .. 7 all at infinity (a whole group at
                           per = 4), product 1 entirely at infinity (FExp = 1)
On the parent commit every packed call returns MLHIP_EINVAL."""
import ctypes
import functools

import pytest

import stream_order_cases as S

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
CASES = {"k1m5": (1, 5), "k3m8": (3, 8), "k13m17": (13, 17), "inf": (2, 9)}
GROUPS = (None, "1", "2", "4")
SWITCHES = ("MLHIP_PAIRING_QUAD", "MLHIP_PAIRING_SAT", "MLHIP_PAIRING_ONE_LANE", "MLHIP_MILLER_GROUP", "MLHIP_G2_PREPARED_GENERAL")


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def _sizes(cid):
    fpb = S.FPB[cid]
    return fpb, 2 * fpb, 4 * fpb, 12 * fpb


@functools.lru_cache(maxsize=None)
def gt_one(cid):
    from oracle import pyref as R

    cp = R.CURVES_BY_ID[cid]
    return R.gt_to_mont_bytes(cp, R.tower(cp).f12_one)


@functools.lru_cache(maxsize=None)
def case(cid, name):
    """(g1, g2, K, m, the oracle's FExp of the K products)"""
    from oracle import cref

    K, m = CASES[name]
    _, g1b, g2b, gtb = _sizes(cid)
    seed = 50 + 7 * cid + 3 * list(CASES).index(name)
    g1, g2 = bytearray(S._pts(cid, 1, seed, K * m)), bytearray(S._pts(cid, 2, seed + 1, K * m))

    def inf1(i):
        g1[i * g1b : (i + 1) * g1b] = bytes(g1b)

    def inf2(i):
        g2[i * g2b : (i + 1) * g2b] = bytes(g2b)

    if name == "inf":
        inf1(0)
        inf1(4), inf2(5), inf1(6), inf2(6), inf1(7)  # pairs 4 .. 7: one side, the other side, both, one side
        for j in range(m, 2 * m):  # product 1: every pair at infinity, the sides alternating
            (inf1 if j % 2 else inf2)(j)
    g1, g2 = bytes(g1), bytes(g2)
    want = cref.final_exp(cid, cref.miller_loop(cid, g1, g2, m, K, 8), K, 8)
    if name == "inf":
        assert want[gtb:] == gt_one(cid) and want[:gtb] != gt_one(cid)
    return g1, g2, K, m, want


def _env(monkeypatch, **values):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in values.items():
        if v is not None:
            monkeypatch.setenv(name, v)


def _dev(data):
    import torch

    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


def _fexp(lib, mlhip, cid, raw, n):
    out = ctypes.create_string_buffer(len(raw))
    mlhip.check(lib.mlhip_final_exp(cid, raw, n, out))
    return out.raw


def miller_host(lib, mlhip, cid, g1, g2, m, K):
    out = ctypes.create_string_buffer(K * _sizes(cid)[3])
    mlhip.check(mlhip.mlhip_miller_loop_products(lib, cid, g1, g2, m, K, out))
    return out.raw


def miller_device(lib, mlhip, cid, g1, g2, m, K):
    import torch

    d1, d2 = _dev(g1), _dev(g2)
    out = torch.full((K * _sizes(cid)[3],), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    mlhip.check(mlhip.mlhip_miller_loop_products_device(lib, cid, d1.data_ptr(), d2.data_ptr(), m, K, out.data_ptr(), st.cuda_stream))
    st.synchronize()
    return _host(out)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("curve", list(CURVES))
def test_products_every_group_size_and_shape(lib, mlhip, curve, name, monkeypatch):
    """MLHIP_MILLER_GROUP unset, 1, 2, 4 x MLHIP_PAIRING_QUAD 0, 1 x host and _device form: FExp of the Miller values is the
    oracle's; the host and the _device form give the same raw bytes"""
    cid = CURVES[curve]
    g1, g2, K, m, want = case(cid, name)
    for quad in ("0", "1"):
        for per in GROUPS:
            _env(monkeypatch, MLHIP_PAIRING_QUAD=quad, MLHIP_MILLER_GROUP=per)
            raw = miller_host(lib, mlhip, cid, g1, g2, m, K)
            assert _fexp(lib, mlhip, cid, raw, K) == want, (curve, name, quad, per, "host")
            assert miller_device(lib, mlhip, cid, g1, g2, m, K) == raw, (curve, name, quad, per, "device")


@pytest.mark.parametrize("family", ["MLHIP_PAIRING_ONE_LANE", "MLHIP_PAIRING_SAT"])
@pytest.mark.parametrize("curve", list(CURVES))
def test_products_second_implementations(lib, mlhip, curve, family, monkeypatch):
    """the one-lane and the saturated lane-pair Miller kernels of the test build take the groups too: every case, every group
    size"""
    cid = CURVES[curve]
    cases = [case(cid, name) for name in CASES]  # the oracle first: its cache is shared
    for per in GROUPS:
        _env(monkeypatch, MLHIP_MILLER_GROUP=per, **{family: "1"})
        assert mlhip.load().mlhip_version() & 0x10000, family  # without the test build the switch would be ignored
        for g1, g2, K, m, want in cases:
            assert _fexp(lib, mlhip, cid, miller_host(lib, mlhip, cid, g1, g2, m, K), K) == want, (curve, family, per, K, m)


def plain_product(lib, mlhip, cid, g1, g2, m, K):
    """the same K products from the library's own calls of at most four pairs: slot-major chunks of four (and a shorter last
    one) through mlhip_miller_loop, multiplied together with mlhip_gt_mul"""
    _, g1b, g2b, gtb = _sizes(cid)
    acc = None
    for lo in range(0, m, 4):
        ppp = min(4, m - lo)
        c1 = b"".join(g1[(k * m + lo) * g1b : (k * m + lo + ppp) * g1b] for k in range(K))
        c2 = b"".join(g2[(k * m + lo) * g2b : (k * m + lo + ppp) * g2b] for k in range(K))
        part = ctypes.create_string_buffer(K * gtb)
        mlhip.check(lib.mlhip_miller_loop(cid, c1, c2, ppp, K, part))
        if acc is None:
            acc = part.raw
        else:
            out = ctypes.create_string_buffer(K * gtb)
            mlhip.check(lib.mlhip_gt_mul(cid, acc, part.raw, K, out))
            acc = out.raw
    return acc


@pytest.mark.parametrize("curve", list(CURVES))
def test_miller_bytes_are_the_exact_product(lib, mlhip, curve, monkeypatch):
    """the Miller value is the exact Fp12 product whatever the grouping: the BYTES of the long call equal the product, by
    mlhip_gt_mul, of the library's plain calls on the same pairs -- for every group size, quads and lane pairs"""
    cid = CURVES[curve]
    for name in ("k13m17", "inf"):
        g1, g2, K, m, _ = case(cid, name)
        for quad in (None, "0"):
            _env(monkeypatch, MLHIP_PAIRING_QUAD=quad)
            want = plain_product(lib, mlhip, cid, g1, g2, m, K)
            for per in GROUPS:
                _env(monkeypatch, MLHIP_PAIRING_QUAD=quad, MLHIP_MILLER_GROUP=per)
                assert miller_host(lib, mlhip, cid, g1, g2, m, K) == want, (curve, name, quad, per)


@pytest.mark.parametrize("curve", list(CURVES))
def test_packed_short_lengths_are_the_plain_call(lib, mlhip, curve, monkeypatch):
    """MLHIP_PRODUCT_PAIRS(m) with m = 1 and m = 4 (and 2, 3): the plain call's bytes, host and _device form"""
    cid = CURVES[curve]
    _env(monkeypatch)
    K = 13
    gtb = _sizes(cid)[3]
    for m in (1, 2, 3, 4):
        g1, g2 = S._pts(cid, 1, 90 + m, K * m), S._pts(cid, 2, 95 + m, K * m)
        plain = ctypes.create_string_buffer(K * gtb)
        mlhip.check(lib.mlhip_miller_loop(cid, g1, g2, m, K, plain))
        assert miller_host(lib, mlhip, cid, g1, g2, m, K) == plain.raw, (curve, m)
        assert miller_device(lib, mlhip, cid, g1, g2, m, K) == plain.raw, (curve, m)


# ---------------------------------------------------------------------------------------------------------------------
# prepared handles
# ---------------------------------------------------------------------------------------------------------------------
Q_INDEX = {5: [2, 0, 2, 1, 1], 9: [1, 1, 0, 2, 0, 2, 2, 1, 0]}  # repeats, every point used


@functools.lru_cache(maxsize=None)
def prepared_case(cid, K, m):
    """(the handle's 3 points, g1 with a planted infinity, the expanded g2, the oracle's FExp)"""
    from oracle import cref

    _, g1b, g2b, _ = _sizes(cid)
    qs = S._pts(cid, 2, 31, 3)
    g1 = bytearray(S._pts(cid, 1, 32 + m + K, K * m))
    g1[(K * m - 2) * g1b : (K * m - 1) * g1b] = bytes(g1b)
    g1 = bytes(g1)
    q = S._chunks(qs, g2b)
    g2 = b"".join(q[j] for j in Q_INDEX[m]) * K
    return qs, g1, g2, cref.final_exp(cid, cref.miller_loop(cid, g1, g2, m, K, 8), K, 8)


@pytest.mark.parametrize("K", [1, 13])
@pytest.mark.parametrize("m", [5, 9])
@pytest.mark.parametrize("curve", list(CURVES))
def test_prepared_products(lib, mlhip, curve, m, K, monkeypatch):
    """a 3-point handle, q_index of length m with repeats: mlhip_miller_loop_prepared after FExp equals the general path and
    the oracle; mlhip_pairing_prepared equals FExp of mlhip_miller_loop_prepared; host and _device forms, every group size,
    quads and lane pairs; q_index = NULL with m > count is MLHIP_EINVAL"""
    import torch

    cid = CURVES[curve]
    gtb = _sizes(cid)[3]
    qs, g1, g2, want = prepared_case(cid, K, m)
    _env(monkeypatch)
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_g2_prepared_create(cid, qs, 3, ctypes.byref(h)))
    try:
        ix = mlhip.q_index_array(Q_INDEX[m], m)
        d1 = _dev(g1)
        for quad in ("0", "1"):
            for per in GROUPS:
                _env(monkeypatch, MLHIP_PAIRING_QUAD=quad, MLHIP_MILLER_GROUP=per)
                tag = (curve, m, K, quad, per)
                general = _fexp(lib, mlhip, cid, miller_host(lib, mlhip, cid, g1, g2, m, K), K)
                assert general == want, tag
                raw = ctypes.create_string_buffer(K * gtb)
                mlhip.check(mlhip.mlhip_miller_loop_prepared_products(lib, h, g1, ix, m, K, raw))
                assert _fexp(lib, mlhip, cid, raw.raw, K) == general, tag
                fused = ctypes.create_string_buffer(K * gtb)
                mlhip.check(mlhip.mlhip_pairing_prepared_products(lib, h, g1, ix, m, K, fused))
                assert fused.raw == general, tag
                st = torch.cuda.current_stream()
                for fn, expect in ((mlhip.mlhip_miller_loop_prepared_products_device, raw.raw),
                                   (mlhip.mlhip_pairing_prepared_products_device, fused.raw)):
                    out = torch.full((K * gtb,), 0xA5, dtype=torch.uint8, device="cuda")
                    mlhip.check(fn(lib, h, d1.data_ptr(), ix, m, K, out.data_ptr(), st.cuda_stream))
                    st.synchronize()
                    assert _host(out) == expect, tag + (fn.__name__,)
        _env(monkeypatch)
        out = ctypes.create_string_buffer(b"\xA5" * (K * gtb), K * gtb)
        for fn in (mlhip.mlhip_miller_loop_prepared_products, mlhip.mlhip_pairing_prepared_products):
            assert fn(lib, h, g1, None, m, K, out) == mlhip.EINVAL  # m > the handle's three points
            assert fn(lib, h, g1, mlhip.q_index_array([3] * m, m), m, K, out) == mlhip.EINVAL  # an index beyond them
        assert out.raw == b"\xA5" * (K * gtb)
    finally:
        lib.mlhip_g2_prepared_destroy(h)


def test_prepared_null_index_takes_point_j(lib, mlhip, monkeypatch):
    """q_index = NULL: slot j takes point j (a 6-point handle, m = 6), the bytes of the explicit index 0 .. 5"""
    cid, m, K = 1, 6, 3
    gtb = _sizes(cid)[3]
    _env(monkeypatch)
    qs, g1 = S._pts(cid, 2, 41, m), S._pts(cid, 1, 42, K * m)
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_g2_prepared_create(cid, qs, m, ctypes.byref(h)))
    try:
        a, b = ctypes.create_string_buffer(K * gtb), ctypes.create_string_buffer(K * gtb)
        mlhip.check(mlhip.mlhip_pairing_prepared_products(lib, h, g1, None, m, K, a))
        mlhip.check(mlhip.mlhip_pairing_prepared_products(lib, h, g1, mlhip.q_index_array(range(m), m), m, K, b))
        general = _fexp(lib, mlhip, cid, miller_host(lib, mlhip, cid, g1, qs * K, m, K), K)
        assert a.raw == b.raw == general
    finally:
        lib.mlhip_g2_prepared_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(lib, mlhip, monkeypatch):
    """packed m = 0, m = 2^32, n * m overflowing and null pointers: MLHIP_EINVAL from all six entry points, host and device
    output buffers as they were; an empty batch returns 0 and writes nothing"""
    import torch

    cid, m, K = 1, 9, 2
    gtb = _sizes(cid)[3]
    _env(monkeypatch)
    g1, g2 = S._pts(cid, 1, 61, K * m), S._pts(cid, 2, 62, K * m)
    d1, d2 = _dev(g1), _dev(g2)
    out = ctypes.create_string_buffer(b"\xA5" * (K * gtb), K * gtb)
    dout = torch.full((K * gtb,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_g2_prepared_create(cid, g2, 3, ctypes.byref(h)))
    try:
        ix = mlhip.q_index_array([0, 1, 2] * 3, m)
        bit63 = 1 << 63
        assert mlhip.product_pairs(0) == bit63 == mlhip.product_pairs(1 << 32)
        for ppp, n in ((bit63, K), (bit63 | (1 << 32), K), (bit63 | (1 << 45) | 9, K), (mlhip.product_pairs(m), 1 << 61),
                       (mlhip.product_pairs((1 << 32) - 1), 1 << 40)):
            prepared_index = ix if (ppp & 0xFFFFFFFF) == m else None  # (an index array is read over all m entries)
            assert lib.mlhip_miller_loop(cid, g1, g2, ppp, n, out) == mlhip.EINVAL, (hex(ppp), n)
            assert lib.mlhip_miller_loop_device(cid, d1.data_ptr(), d2.data_ptr(), ppp, n, dout.data_ptr(), st) == mlhip.EINVAL
            for fn in (lib.mlhip_miller_loop_prepared, lib.mlhip_pairing_prepared):
                assert fn(h, g1, prepared_index, ppp, n, out) == mlhip.EINVAL, (hex(ppp), n)
            for fn in (lib.mlhip_miller_loop_prepared_device, lib.mlhip_pairing_prepared_device):
                assert fn(h, d1.data_ptr(), prepared_index, ppp, n, dout.data_ptr(), st) == mlhip.EINVAL, (hex(ppp), n)
        pk = mlhip.product_pairs(m)
        for a1, a2, o in ((None, g2, out), (g1, None, out), (g1, g2, None)):
            assert lib.mlhip_miller_loop(cid, a1, a2, pk, K, o) == mlhip.EINVAL
        for a1, a2, o in ((None, d2.data_ptr(), dout.data_ptr()), (d1.data_ptr(), None, dout.data_ptr()), (d1.data_ptr(), d2.data_ptr(), None)):
            assert lib.mlhip_miller_loop_device(cid, a1, a2, pk, K, o, st) == mlhip.EINVAL
        for fn in (lib.mlhip_miller_loop_prepared, lib.mlhip_pairing_prepared):
            assert fn(h, None, ix, pk, K, out) == mlhip.EINVAL and fn(h, g1, ix, pk, K, None) == mlhip.EINVAL
            assert fn(None, g1, ix, pk, K, out) == mlhip.EINVAL
            assert fn(h, g1, ix, pk, 0, out) == 0
        for fn in (lib.mlhip_miller_loop_prepared_device, lib.mlhip_pairing_prepared_device):
            assert fn(h, None, ix, pk, K, dout.data_ptr(), st) == mlhip.EINVAL and fn(h, d1.data_ptr(), ix, pk, K, None, st) == mlhip.EINVAL
            assert fn(h, d1.data_ptr(), ix, pk, 0, dout.data_ptr(), st) == 0
        assert lib.mlhip_miller_loop(cid, g1, g2, pk, 0, out) == 0
        assert lib.mlhip_miller_loop_device(cid, d1.data_ptr(), d2.data_ptr(), pk, 0, dout.data_ptr(), st) == 0
        assert lib.mlhip_miller_loop(cid, g1, g2, 9, K, out) == mlhip.EINVAL  # a plain 9 stays what it was
        torch.cuda.synchronize()
        assert out.raw == b"\xA5" * (K * gtb) and _host(dout) == b"\xA5" * (K * gtb)
    finally:
        lib.mlhip_g2_prepared_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# the three _device forms on a busy stream (tests/stream_order_cases.py: the scenario of tests/test_stream_order_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
class LongMiller(S.Case):
    """mlhip_miller_loop_products_device: K products of m = 9 pairs"""

    def __init__(self, cid, K=11, m=9, seed=0):
        self.cid, self.K, self.m = cid, K, m
        self.gtb = 12 * S.FPB[cid]
        self.real = [S._pts(cid, 1, 70 + seed, K * m), S._pts(cid, 2, 71 + seed, K * m)]
        self.decoy = [S._pts(cid, 1, 72 + seed, K * m), S._pts(cid, 2, 73 + seed, K * m)]
        self.out_bytes = [self.gtb * K]

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(mlhip.mlhip_miller_loop_products_device(lib, self.cid, ins[0], ins[1], self.m, self.K, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.gtb * self.K)
        mlhip.check(mlhip.mlhip_miller_loop_products(lib, self.cid, ins[0], ins[1], self.m, self.K, out))
        return [out.raw]

    def oracle(self, ins, host):
        cref = S._cref()
        return [cref.final_exp(self.cid, cref.miller_loop(self.cid, ins[0], ins[1], self.m, self.K, 8), self.K, 8)]

    def canon(self, lib, mlhip, outs):
        return [_fexp(lib, mlhip, self.cid, outs[0], self.K)]


class LongPrepared(S.Prepared):
    """mlhip_miller_loop_prepared_products_device / mlhip_pairing_prepared_products_device: 3 prepared points, m = 9 pairs per
    product, q_index (9 host entries) overwritten as soon as the call returns"""

    def __init__(self, cid, fused, K=11, m=9):
        S.Prepared.__init__(self, cid, fused, n=K, m=3, ppp=m)
        self.host_real = {"q_index": (ctypes.c_uint32, Q_INDEX[9])}
        self.host_other = {"q_index": (ctypes.c_uint32, [2 - j for j in Q_INDEX[9]])}

    def call(self, lib, mlhip, ins, outs, host, stream):
        fn = mlhip.mlhip_pairing_prepared_products_device if self.fused else mlhip.mlhip_miller_loop_prepared_products_device
        mlhip.check(fn(lib, self.h, ins[0], host["q_index"], self.ppp, self.n, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.gtb * self.n)
        fn = mlhip.mlhip_pairing_prepared_products if self.fused else mlhip.mlhip_miller_loop_prepared_products
        mlhip.check(fn(lib, self.h, ins[0], host["q_index"], self.ppp, self.n, out))
        return [out.raw]


@pytest.fixture(scope="module")
def delay(lib, mlhip):
    d = S.Delay(lib, mlhip)
    assert 50.0 <= d.ms <= 2000.0, (d.repeat, d.ms)
    return d


BUSY = {"miller": lambda: LongMiller(1), "miller_prepared": lambda: LongPrepared(1, False), "pairing_prepared": lambda: LongPrepared(2, True)}


@pytest.mark.parametrize("form", list(BUSY))
def test_busy_stream(lib, mlhip, delay, form, monkeypatch):
    """inputs still being produced on the stream in front of the call, inputs and q_index overwritten right behind it, the
    call back on the host long before the stream has drained"""
    import torch

    _env(monkeypatch)
    log = []
    S.run_scenario(lib, mlhip, BUSY[form](), torch.cuda.Stream(), delay, log.append, "products/" + form)


def test_two_streams_share_the_scratch(lib, mlhip, delay, monkeypatch):
    """call A behind the delay on s1, call B at once on the idle s2, call C on s1 again: one scratch buffer, chained by its
    event.  B is the largest and warms the scratch up, so nothing is regrown between the calls."""
    import torch

    _env(monkeypatch)
    cid = 1
    cases = [LongMiller(cid, 11, 9, 0), LongMiller(cid, 14, 9, 4), LongMiller(cid, 11, 9, 8)]
    ins = [[_dev(b) for b in c.real] for c in cases]
    outs = [torch.full((c.out_bytes[0],), 0xA5, dtype=torch.uint8, device="cuda") for c in cases]
    want = [c.oracle(c.real, {})[0] for c in cases]
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    s2 = delay.independent_stream(s1)
    delay.clear()
    cases[1].call(lib, mlhip, S._ptrs(ins[1]), [outs[1].data_ptr()], {}, s2.cuda_stream)
    torch.cuda.synchronize()
    assert cases[1].canon(lib, mlhip, [_host(outs[1])])[0] == want[1]
    outs[1].fill_(0xA5)
    torch.cuda.synchronize()
    delay.queue(s1)
    for c, i, o, s in zip(cases, ins, outs, (s1, s2, s1)):
        c.call(lib, mlhip, S._ptrs(i), [o.data_ptr()], {}, s.cuda_stream)
    busy = not s1.query()
    s1.synchronize()
    s2.synchronize()
    delay.check()
    assert busy, "the three calls returned only after the first stream had drained"
    for tag, c, o, w in zip("ABC", cases, outs, want):
        assert c.canon(lib, mlhip, [_host(o)])[0] == w, "call " + tag
