"""Every pairing path against the oracle (oracle/cref, byte-exact; oracle/pyref for Gt.Exp).

pairing_device (mathlib_amd/csrc/pairing_kernels.h) picks a kernel from what is asked (Miller loop, final exponentiation,
fused pairing), the pairs per product (1 .. 4), the curve and the batch size; mlhip_pairing_product (api_pairing.hip) groups four
pairs per Miller loop from 2^17 pairs on.  The points are P_i = [a_i]G1 and Q_i = [b_i]G2 with known logs
(cref.gen_points), so any product of pairings has an exact expected value: e(G1, G2)^S with S = sum a_i b_i mod r is ONE
oracle pairing of [S]G1 with G2.  Raw Miller values are not canonical; they are compared after a final exponentiation."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
# the kernel families a test can force: quads (pairing_quad.h), lane pairs (carry-free; BN254's Miller loop: the saturated
# lane pairs), the saturated lane pairs and one lane per pairing (the last two: test build only)
FAMILIES = {
    "quad": ("MLHIP_PAIRING_QUAD", "1"),
    "pairs": ("MLHIP_PAIRING_QUAD", "0"),
    "sat": ("MLHIP_PAIRING_SAT", "1"),
    "one_lane": ("MLHIP_PAIRING_ONE_LANE", "1"),
}
ALT_FAMILIES = ("sat", "one_lane")
SWITCHES = ("MLHIP_PAIRING_QUAD", "MLHIP_PAIRING_SAT", "MLHIP_PAIRING_ONE_LANE")


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def _cp(cid):
    from oracle import pyref as R

    return R.CURVES_BY_ID[cid]


def _sizes(cid):
    fpb = 32 if cid == 0 else 48
    return fpb, 2 * fpb, 4 * fpb, 12 * fpb


@functools.lru_cache(maxsize=None)
def gt_one(cid):
    from oracle import pyref as R

    cp = _cp(cid)
    return R.gt_to_mont_bytes(cp, R.tower(cp).f12_one)


@functools.lru_cache(maxsize=None)
def generators(cid):
    from oracle import cref

    return cref.gen_points(cid, 1, 1, 0, 1), cref.gen_points(cid, 2, 1, 0, 1)


def gen_pow(cid, s):
    """e(G1, G2)^s by the oracle: one pairing of [s]G1 with G2"""
    from oracle import cref

    g1, g2 = generators(cid)
    return cref.pairing_batch(cid, cref.point_mul(cid, 1, g1, s % _cp(cid).r), g2, 1, 1)


class Pairs:
    """n pairs (P_i, Q_i) = ([a_i]G1, [b_i]G2) as byte arrays in the C-ABI layout, with their discrete logs"""

    def __init__(self, cid, n, seed):
        from oracle import cref

        self.cid, self.n = cid, n
        r = _cp(cid).r
        rng = np.random.default_rng(seed)
        k0, k1, m0, m1 = (int(v) for v in rng.integers(1, 1 << 62, size=4))
        self.g1 = bytearray(cref.gen_points(cid, 1, k0, k1, n))
        self.g2 = bytearray(cref.gen_points(cid, 2, m0, m1, n))
        self.a = [(k0 + i * k1) % r for i in range(n)]
        self.b = [(m0 + i * m1) % r for i in range(n)]
        _, self.g1b, self.g2b, self.gtb = _sizes(cid)

    def g1_inf(self, i):
        self.g1[i * self.g1b : (i + 1) * self.g1b] = bytes(self.g1b)
        self.a[i] = 0

    def g2_inf(self, i):
        self.g2[i * self.g2b : (i + 1) * self.g2b] = bytes(self.g2b)
        self.b[i] = 0

    def neg_of(self, dst, src):
        """pair dst = (-P_src, Q_src)"""
        from oracle import pyref as R

        cp = _cp(self.cid)
        p = R.g1_from_mont_bytes(cp, bytes(self.g1[src * self.g1b : (src + 1) * self.g1b]))
        self.g1[dst * self.g1b : (dst + 1) * self.g1b] = R.g1_to_mont_bytes(cp, R.g1_neg(cp, p))
        self.g2[dst * self.g2b : (dst + 1) * self.g2b] = self.g2[src * self.g2b : (src + 1) * self.g2b]
        self.a[dst], self.b[dst] = (-self.a[src]) % cp.r, self.b[src]

    def copy(self, dst, src):
        self.g1[dst * self.g1b : (dst + 1) * self.g1b] = self.g1[src * self.g1b : (src + 1) * self.g1b]
        self.g2[dst * self.g2b : (dst + 1) * self.g2b] = self.g2[src * self.g2b : (src + 1) * self.g2b]
        self.a[dst], self.b[dst] = self.a[src], self.b[src]

    def p1(self, lo, hi):
        return bytes(self.g1[lo * self.g1b : hi * self.g1b])

    def p2(self, lo, hi):
        return bytes(self.g2[lo * self.g2b : hi * self.g2b])

    def gather(self, products, ppp):
        """the pairs of these products (ppp consecutive pairs each), as two byte strings"""
        return (b"".join(self.p1(j * ppp, (j + 1) * ppp) for j in products),
                b"".join(self.p2(j * ppp, (j + 1) * ppp) for j in products))

    def exponents(self, ppp, n_products):
        r = _cp(self.cid).r
        return [sum(self.a[j * ppp + k] * self.b[j * ppp + k] for k in range(ppp)) % r for j in range(n_products)]


def _gt(buf, j, gtb):
    return buf[j * gtb : (j + 1) * gtb]


def _family(monkeypatch, mlhip, family):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if family is None:
        return
    name, value = FAMILIES[family]
    monkeypatch.setenv(name, value)
    if family in ALT_FAMILIES:
        # the switch exists in the test build only: without this, a routing slip would re-run the default path and pass
        assert mlhip.load().mlhip_version() & 0x10000, family


# ---------------------------------------------------------------------------------------------------------------------
# (a) every kernel family forced, pairs per product 1 .. 4, a small ragged batch with planted infinities
# ---------------------------------------------------------------------------------------------------------------------
N_SMALL = 83  # ragged: the last wave of quads / lane pairs is partly idle


@functools.lru_cache(maxsize=None)
def small_case(cid, ppp):
    """(pairs, oracle raw Miller values, their FExp, the fused pairings of all n * ppp pairs), computed once per (curve, ppp)"""
    from oracle import cref

    n = N_SMALL
    pr = Pairs(cid, n * ppp, 1000 + 10 * cid + ppp)
    for k in range(ppp):  # G1 at infinity in slot k of product 1 + k
        pr.g1_inf((1 + k) * ppp + k)
    pr.g2_inf(10 * ppp + ppp - 1)  # G2 at infinity (last slot of product 10)
    for k in range(ppp):  # product 20: every pair at infinity, G1 and G2 alternating; product 21: every G1
        (pr.g1_inf if k % 2 == 0 else pr.g2_inf)(20 * ppp + k)
        pr.g1_inf(21 * ppp + k)
    if ppp >= 2:
        pr.neg_of(30 * ppp + 1, 30 * ppp)  # (P, Q) next to (-P, Q): one
        if ppp == 3:
            pr.g2_inf(30 * ppp + 2)
        if ppp == 4:
            pr.neg_of(30 * ppp + 3, 30 * ppp + 2)
        pr.copy(40 * ppp + 1, 40 * ppp)  # the same pair twice
    pr.g1_inf(n * ppp - 1)  # an infinity in the last, ragged product
    g1, g2 = bytes(pr.g1), bytes(pr.g2)
    raw = cref.miller_loop(cid, g1, g2, ppp, n, 8)
    fe = cref.final_exp(cid, raw, n, 8)
    fused = cref.pairing_batch(cid, g1, g2, n * ppp, 8)
    gtb = pr.gtb
    one = gt_one(cid)
    assert _gt(fe, 20, gtb) == one and _gt(fe, 21, gtb) == one
    if ppp >= 2:
        assert _gt(fe, 30, gtb) == one
    # the identity checks the oracle itself on a few products
    exps = pr.exponents(ppp, n)
    for j in (0, 1, 40, n - 1):
        assert _gt(fe, j, gtb) == gen_pow(cid, exps[j]), (ppp, j)
    return pr, raw, fe, fused


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("curve", list(CURVES))
def test_pairing_family_matrix(lib, mlhip, curve, family, monkeypatch):
    """Miller loop (after the oracle's FExp), FExp of the oracle's raw Miller values and the fused pairing, ppp = 1 .. 4,
    on one kernel family forced by its switch"""
    from oracle import cref

    cid = CURVES[curve]
    gtb = _sizes(cid)[3]
    n = N_SMALL
    cases = [small_case(cid, ppp) for ppp in (1, 2, 3, 4)]  # the oracle first: its cache is shared by the families
    _family(monkeypatch, mlhip, family)
    for ppp, (pr, raw, fe, fused) in zip((1, 2, 3, 4), cases):
        g1, g2 = bytes(pr.g1), bytes(pr.g2)
        ml = ctypes.create_string_buffer(gtb * n)
        mlhip.check(lib.mlhip_miller_loop(cid, g1, g2, ppp, n, ml))
        got = cref.final_exp(cid, ml.raw, n, 8)
        bad = [j for j in range(n) if _gt(got, j, gtb) != _gt(fe, j, gtb)]
        assert not bad, ("miller_loop", family, ppp, bad)
        out = ctypes.create_string_buffer(gtb * n)
        mlhip.check(lib.mlhip_final_exp(cid, raw, n, out))
        bad = [j for j in range(n) if _gt(out.raw, j, gtb) != _gt(fe, j, gtb)]
        assert not bad, ("final_exp", family, ppp, bad)
        out = ctypes.create_string_buffer(gtb * n * ppp)
        mlhip.check(lib.mlhip_pairing_batch(cid, g1, g2, n * ppp, out))
        bad = [j for j in range(n * ppp) if _gt(out.raw, j, gtb) != _gt(fused, j, gtb)]
        assert not bad, ("pairing_batch", family, ppp, bad)


# ---------------------------------------------------------------------------------------------------------------------
# shared large inputs: (b) the default selection across the size switches and 2. mlhip_pairing_product's grouped path
# ---------------------------------------------------------------------------------------------------------------------
N_LARGE = 4 * ((1 << 15) + 1)  # = 2^17 + 4: four pairs per element at the largest switch, and every pairing_product size
G1_INF = (5, 12, 13, 14, 15, 31, 40, 50, 55, 56, 57, 58, 59, 4 * (1 << 14) - 1, 4 * (1 << 14) + 3, 4 * (1 << 15) - 1,
          4 * (1 << 15) + 3)
G2_INF = (38, 45, 77, (1 << 14) - 1, 1 << 14, (1 << 15) - 1, 1 << 15, (1 << 17) + 1)


@functools.lru_cache(maxsize=None)
def large_pairs(cid):
    """2^17 + 4 pairs with planted infinities: single ones, a whole quadruple (56 .. 59), slot 3 of a quadruple (31, 55),
    the last element of each batch size below; (-P, Q) at 84 next to (P, Q) at 83, across a group boundary of four"""
    pr = Pairs(cid, N_LARGE, 77 + cid)
    for i in G1_INF:
        pr.g1_inf(i)
    for i in G2_INF:
        pr.g2_inf(i)
    pr.neg_of(84, 83)
    return pr


def _upload(data):
    import torch

    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def weighted_product(lib, mlhip, cid, outs, n, seed):
    """(prod_j outs_j^(w_j), w) with random 64-bit w_j: mlhip_gt_exp_device, then a tree of mlhip_gt_mul_device"""
    import torch

    gtb = _sizes(cid)[3]
    w = np.zeros((n, 4), dtype=np.uint64)
    w[:, 0] = np.random.default_rng(seed).integers(1, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    st = torch.cuda.current_stream().cuda_stream
    d_in = _upload(outs[: n * gtb])
    d_w = _upload(w.tobytes())
    buf = torch.empty_like(d_in)
    mlhip.check(lib.mlhip_gt_exp_device(cid, d_in.data_ptr(), d_w.data_ptr(), 0, n, buf.data_ptr(), st))
    m = n
    while m > 1:
        half = m // 2
        mlhip.check(lib.mlhip_gt_mul_device(cid, buf.data_ptr(), buf.data_ptr() + (m - half) * gtb, half, buf.data_ptr(), st))
        m -= half
    torch.cuda.synchronize()
    return bytes(buf[:gtb].cpu().numpy().tobytes()), [int(x) for x in w[:, 0]]


def check_identity(lib, mlhip, cid, outs, exps, seed, what):
    """prod_j out_j^(w_j) == e(G1, G2)^(sum_j w_j e_j): covers every output (a wrong, missing or permuted one changes it)"""
    left, w = weighted_product(lib, mlhip, cid, outs, len(exps), seed)
    right = gen_pow(cid, sum(wj * e for wj, e in zip(w, exps)))
    assert left == right, what


SWITCH_SIZES = [("BLS12-381", 1 << 14), ("BLS12-381", (1 << 14) + 1), ("BN254", 1 << 14), ("BN254", (1 << 14) + 1),
                ("BLS12-377", 1 << 15), ("BLS12-377", (1 << 15) + 1)]


@pytest.mark.parametrize("curve,n", SWITCH_SIZES, ids=["%s-%d" % c for c in SWITCH_SIZES])
def test_default_selection_across_size_switch(lib, mlhip, curve, n, monkeypatch):
    """no switch set: quads up to 2^14 elements (2^15 on BLS12-377), lane pairs above (BN254's Miller loop: the saturated
    lane pairs; BLS12-377's Miller loop: quads at every size) -- just below and just above each switch, the Miller loop at
    ppp = 1 and 4 (after mlhip_final_exp), mlhip_final_exp and the fused pairing, every output through the weighted-product
    identity, a sample, the ragged last wave and the planted infinities byte for byte against the oracle"""
    from oracle import cref

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    cid = CURVES[curve]
    gtb = _sizes(cid)[3]
    pr = large_pairs(cid)
    ml1 = ctypes.create_string_buffer(gtb * n)
    mlhip.check(lib.mlhip_miller_loop(cid, pr.p1(0, n), pr.p2(0, n), 1, n, ml1))
    fe1 = ctypes.create_string_buffer(gtb * n)  # mlhip_final_exp at this size, on the GPU's raw Miller values
    mlhip.check(lib.mlhip_final_exp(cid, ml1.raw, n, fe1))
    pb = ctypes.create_string_buffer(gtb * n)
    mlhip.check(lib.mlhip_pairing_batch(cid, pr.p1(0, n), pr.p2(0, n), n, pb))
    ml4 = ctypes.create_string_buffer(gtb * n)
    mlhip.check(lib.mlhip_miller_loop(cid, pr.p1(0, 4 * n), pr.p2(0, 4 * n), 4, n, ml4))
    fe4 = ctypes.create_string_buffer(gtb * n)
    mlhip.check(lib.mlhip_final_exp(cid, ml4.raw, n, fe4))

    e1, e4 = pr.exponents(1, n), pr.exponents(4, n)
    check_identity(lib, mlhip, cid, fe1.raw, e1, 1, "miller_loop ppp=1 + final_exp")
    check_identity(lib, mlhip, cid, pb.raw, e1, 2, "pairing_batch")
    check_identity(lib, mlhip, cid, fe4.raw, e4, 3, "miller_loop ppp=4 + final_exp")

    planted1 = sorted({i for i in G1_INF + G2_INF + (83, 84) if i < n})
    planted4 = sorted({i // 4 for i in G1_INF + G2_INF + (83, 84) if i < 4 * n})
    tail = list(range(n - 8, n))
    idx1 = sorted(set(range(0, n, n // 32)) | set(tail) | set(planted1))
    idx4 = sorted(set(range(0, n, n // 32)) | set(tail) | set(planted4))
    q1, q2 = pr.gather(idx1, 1)
    want1 = cref.pairing_batch(cid, q1, q2, len(idx1), 8)
    for k, j in enumerate(idx1):
        assert _gt(pb.raw, j, gtb) == _gt(want1, k, gtb), ("pairing_batch", j)
        assert _gt(fe1.raw, j, gtb) == _gt(want1, k, gtb), ("miller_loop ppp=1", j)
    q1, q2 = pr.gather(idx4, 4)
    want4 = cref.final_exp(cid, cref.miller_loop(cid, q1, q2, 4, len(idx4), 8), len(idx4), 8)
    for k, j in enumerate(idx4):
        assert _gt(fe4.raw, j, gtb) == _gt(want4, k, gtb), ("miller_loop ppp=4", j)
    assert _gt(fe4.raw, 14, gtb) == gt_one(cid)  # pairs 56 .. 59: every one at infinity


# ---------------------------------------------------------------------------------------------------------------------
# (c) Gt.Exp: scalar forms (plain / Montgomery, not reduced) on every family, on a Gt element and on a raw Miller value
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gt_exp_case(cid):
    """(inputs, scalars, expected) for scalars_mont = 0 and 1: pyref's x^(s mod r), x^(s 2^-256 mod r)"""
    from oracle import cref
    from oracle import pyref as R

    cp = _cp(cid)
    T = R.tower(cp)
    pr = Pairs(cid, 1, 4242 + cid)
    x_gt = cref.pairing_batch(cid, pr.p1(0, 1), pr.p2(0, 1), 1, 1)
    x_raw = cref.miller_loop(cid, pr.p1(0, 1), pr.p2(0, 1), 1, 1, 1)
    rng = np.random.default_rng(99 + cid)
    rand = [int.from_bytes(rng.bytes(32), "little") for _ in range(2)]
    scalars = [0, 1, cp.r - 1, cp.r, cp.r + 1, 2 * cp.r + 3, (1 << 256) - 1] + rand
    rinv = pow(1 << 256, -1, cp.r)
    inputs = [x_gt, x_raw]
    res = {}
    for mont in (0, 1):
        ins, scs, want = [], [], []
        for x in inputs:
            xf = R.gt_from_mont_bytes(cp, x)
            for s in scalars:
                e = s % cp.r if mont == 0 else s * rinv % cp.r
                ins.append(x)
                scs.append(s.to_bytes(32, "little"))
                want.append(R.gt_to_mont_bytes(cp, T.f12_pow(xf, e)))
        res[mont] = (b"".join(ins), b"".join(scs), want)
    return res


@pytest.mark.parametrize("family", [None, "pairs", "sat", "one_lane"], ids=["quad", "pairs", "sat", "one_lane"])
@pytest.mark.parametrize("curve", list(CURVES))
def test_gt_exp_scalar_forms(lib, mlhip, curve, family, monkeypatch):
    """scalars 0, 1, r - 1, r, r + 1, 2r + 3, 2^256 - 1 and random 256-bit ones, plain and Montgomery: reduced mod r on the
    device (include/mlhip.h: as for the MSM entry points) -- for a raw Miller value too, which is not of order r"""
    cid = CURVES[curve]
    gtb = _sizes(cid)[3]
    case = gt_exp_case(cid)
    _family(monkeypatch, mlhip, family)
    for mont in (0, 1):
        ins, scs, want = case[mont]
        m = len(want)
        out = ctypes.create_string_buffer(gtb * m)
        mlhip.check(lib.mlhip_gt_exp(cid, ins, scs, mont, m, out))
        bad = [j for j in range(m) if _gt(out.raw, j, gtb) != want[j]]
        assert not bad, (family, mont, bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. mlhip_pairing_product (the verifier's entry point) against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", list(CURVES))
def test_pairing_product_small(lib, mlhip, curve, monkeypatch):
    """n = 0 .. 64 pairs, one Miller loop per pair and a Gt tree: FExp(prod_i MillerLoop(P_i, Q_i)) from the oracle's
    Miller loop over all n pairs (cref takes any ppp); the empty product is one"""
    from oracle import cref

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    cid = CURVES[curve]
    gtb = _sizes(cid)[3]
    pr = Pairs(cid, 64, 500 + cid)
    pr.g1_inf(2)
    pr.g2_inf(16)
    pr.neg_of(40, 39)
    out = ctypes.create_string_buffer(gtb)
    mlhip.check(lib.mlhip_pairing_product(cid, None, None, 0, out))
    assert out.raw == gt_one(cid)
    for n in (1, 2, 3, 4, 5, 17, 64):
        g1, g2 = pr.p1(0, n), pr.p2(0, n)
        mlhip.check(lib.mlhip_pairing_product(cid, g1, g2, n, out))
        want = cref.final_exp(cid, cref.miller_loop(cid, g1, g2, n, 1, 8), 1, 8)
        assert out.raw == want, n
        assert want == gen_pow(cid, pr.exponents(n, 1)[0]), n


PRODUCT_SIZES = [("BLS12-381", (1 << 17) - 1), ("BLS12-381", 1 << 17), ("BLS12-381", (1 << 17) + 1), ("BLS12-381", (1 << 17) + 3),
                 ("BN254", (1 << 17) + 3), ("BLS12-377", (1 << 17) + 3)]


@pytest.mark.parametrize("curve,n", PRODUCT_SIZES, ids=["%s-%d" % c for c in PRODUCT_SIZES])
def test_pairing_product_grouped(lib, mlhip, curve, n, monkeypatch):
    """from 2^17 pairs on, groups of four pairs per Miller loop (lp28 on BLS12-381, quads on BLS12-377, saturated lane
    pairs on BN254) plus a tail product of the 1 .. 3 pairs left and a Gt tree: against e(G1, G2)^(sum a_i b_i); the
    planted infinities sit in every slot of some groups, in a whole group and in the tail, and (-P, Q) straddles a group
    boundary.  2^17 + 1 is verifier-shaped: its tail pair is ([-S]G1, G2), so the exact result is one."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    cid = CURVES[curve]
    gtb = _sizes(cid)[3]
    pr = large_pairs(cid)
    out = ctypes.create_string_buffer(gtb)
    if n == (1 << 17) + 1:
        from oracle import cref

        m = 1 << 17
        s = sum(pr.exponents(1, m)) % _cp(cid).r
        g1_gen, g2_gen = generators(cid)
        g1 = pr.p1(0, m) + cref.point_mul(cid, 1, g1_gen, (-s) % _cp(cid).r)
        g2 = pr.p2(0, m) + g2_gen
        mlhip.check(lib.mlhip_pairing_product(cid, g1, g2, n, out))
        assert out.raw == gt_one(cid)
        return
    mlhip.check(lib.mlhip_pairing_product(cid, pr.p1(0, n), pr.p2(0, n), n, out))
    assert out.raw == gen_pow(cid, sum(pr.exponents(1, n)))
