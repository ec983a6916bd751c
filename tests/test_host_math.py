"""The kernels' __host__ __device__ math (mathlib_amd/csrc/*.h), compiled for the CPU with the 32-bit
device code path forced (tests/hostmath), against oracle/pyref.py.  This is how the field / curve /
pairing formulas and the per-thread MSM bodies are checked in the GPU-less container; the same
functions then run inside the HIP kernels, which the -m gpu tests check through the C ABI."""
import ctypes
import random

import pytest

from conftest import load_golden
from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]


def fpb(cp, a):
    return R.fp_to_mont_bytes(cp, a)


@pytest.mark.parametrize("name", CURVES)
def test_fp_ops(hostmath, name):
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("hm/fp/" + name)
    pairs = [(d.below(cp.p), d.below(cp.p)) for _ in range(30)] + [(0, 0), (cp.p - 1, cp.p - 1), (0, cp.p - 1), (1, cp.p - 1), (2, (cp.p + 1) // 2)]
    for a, b in pairs:
        out = ctypes.create_string_buffer(n)
        ops = [(0, a * b % cp.p), (1, (a + b) % cp.p), (2, (a - b) % cp.p), (3, (-a) % cp.p), (5, a * a % cp.p), (6, a * pow(2, -1, cp.p) % cp.p)]
        if a:
            ops.append((4, pow(a, -1, cp.p)))
        for op, exp in ops:
            assert L.hm_fp_op(cid, op, fpb(cp, a), fpb(cp, b), out) == 0
            assert R.fp_from_mont_bytes(cp, out.raw) == exp, (name, op, a, b)


@pytest.mark.parametrize("name", CURVES)
def test_fp12_tower(hostmath, name):
    cp = R.CURVES[name]
    T = R.tower(cp)
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("hm/f12/" + name)
    rf = lambda: tuple((d.below(cp.p), d.below(cp.p)) for _ in range(6))  # noqa: E731
    gb = lambda f: R.gt_to_mont_bytes(cp, f)  # noqa: E731
    out = ctypes.create_string_buffer(12 * n)
    for _ in range(2):
        f, g = rf(), rf()
        for op, exp in ((0, T.f12_mul(f, g)), (1, T.f12_sqr(f)), (2, T.f12_inv(f)), (3, T.f12_frob(f, 1)), (4, T.f12_frob(f, 2)), (5, T.f12_frob(f, 3)), (7, T.f12_conj(f))):
            assert L.hm_fp12_op(cid, op, gb(f), gb(g), out) == 0
            assert R.gt_from_mont_bytes(cp, out.raw) == exp, (name, op)
        c = T.f12_mul(T.f12_conj(f), T.f12_inv(f))
        c = T.f12_mul(T.f12_frob(c, 2), c)  # cyclotomic subgroup element
        L.hm_fp12_op(cid, 6, gb(c), None, out)
        assert R.gt_from_mont_bytes(cp, out.raw) == T.f12_sqr(c)
        L.hm_fp12_op(cid, 8, gb(c), None, out)
        assert R.gt_from_mont_bytes(cp, out.raw) == T.f12_pow(c, cp.x)
        L.hm_fp12_op(cid, 9, gb(f), None, out)
        assert R.gt_from_mont_bytes(cp, out.raw) == R.final_exp(cp, f)
    # the unit (pairings with a point at infinity): the compressed-squaring chain must survive B = C = 0
    one = T.f12_one
    for op in (8, 9):
        L.hm_fp12_op(cid, op, gb(one), None, out)
        assert R.gt_from_mont_bytes(cp, out.raw) == one


@pytest.mark.parametrize("name", CURVES)
def test_host_tail_horner_in_jacobian_coordinates(hostmath, name):
    """ec_jac.h (round 4): the Horner pass of an MSM's host tail, sum_w 2^off[w] V[w], in Jacobian coordinates (dbl-2009-l,
    add-2007-bl, XYZZ <-> Jacobian without an inversion) against the XYZZ pass it replaces and against Python integers:
    G1 and G2, window sums that are infinity, equal (the addition's doubling branch: 2 V + V after one doubling of V),
    opposite, uneven window widths."""
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("hm/horner/" + name)
    for group in (1, 2):
        rand, add, neg, mul = (R.random_g1, R.g1_add, R.g1_neg, R.g1_mul_unreduced) if group == 1 else (R.random_g2, R.g2_add, R.g2_neg, R.g2_mul_unreduced)
        enc = R.g1_to_mont_bytes if group == 1 else R.g2_to_mont_bytes
        dec = R.g1_from_mont_bytes if group == 1 else R.g2_from_mont_bytes
        size = (2 if group == 1 else 4) * n
        p, q = rand(cp, d), rand(cp, d)
        cases = [
            ([rand(cp, d) for _ in range(16)], [0] + [16] * 15),
            ([rand(cp, d) for _ in range(5)], [0, 3, 1, 7, 2]),
            ([None, p, None, q, None], [0, 2, 2, 1, 5]),
            ([p, p], [0, 1]),               # 2 p + p
            ([mul(cp, p, 2), neg(cp, p)], [0, 1]),   # 2 (-p) + 2 p = infinity
            ([add(cp, p, p), p], [0, 1]),   # acc = 2 p after the doubling, then + 2 p: the addition's doubling branch
            ([None, None, None], [0, 4, 4]),
            ([q], [0]),
        ]
        for V, down in cases:
            want = None
            for w in range(len(V) - 1, -1, -1):
                want = add(cp, want, V[w])
                if down[w]:
                    want = mul(cp, want, 1 << down[w])
            buf = b"".join(enc(cp, v) for v in V)
            dn = (ctypes.c_int * len(V))(*down)
            for which in (0, 1):
                out = ctypes.create_string_buffer(size)
                assert L.hm_horner(cid, group, buf, len(V), dn, which, out) == 0
                assert dec(cp, out.raw) == want, (name, group, down, which)


@pytest.mark.parametrize("name", CURVES)
def test_shifted_base_tables_msm_on_the_host(hostmath, name):
    """msm_fold.h (round 4): a whole MSM over shifted-base tables replayed with the kernels' own bodies (hm_fold_msm: table
    rows 2^off(j) P_i by Jacobian doublings, all signed digits into ONE bucket set, bucket groups reduced like windows, the
    groups combined into one window by k_group_combine_q's selection, that window's host tail) against sum_i [s_i] P_i in
    Python integers: G1 and G2, one bucket group and several, digit widths that divide the scalar unevenly, scalars 0 / 1 /
    r - 1 / equal, a base at infinity."""
    cp = R.CURVES[name]
    L, cid, fb = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("hm/fold/" + name)
    for group in (1, 2):
        rand, add, mul = (R.random_g1, R.g1_add, R.g1_mul_unreduced) if group == 1 else (R.random_g2, R.g2_add, R.g2_mul_unreduced)
        enc = R.g1_to_mont_bytes if group == 1 else R.g2_to_mont_bytes
        dec = R.g1_from_mont_bytes if group == 1 else R.g2_from_mont_bytes
        size = (2 if group == 1 else 4) * fb
        n = 14 if group == 1 else 6
        pts = [rand(cp, d) for _ in range(n)]
        pts[3] = None
        sc = [d.below(cp.r) for _ in range(n)]
        sc[0], sc[1], sc[2], sc[4], sc[5] = 0, 1, cp.r - 1, sc[n - 1], (1 << 200) - 1
        want = None
        for p, k in zip(pts, sc):
            if p is not None and k:
                want = add(cp, want, mul(cp, p, k))
        buf = b"".join(enc(cp, p) for p in pts)
        sb = b"".join(k.to_bytes(32, "little") for k in sc)
        for c, lgM, lgL in ((7, 4, 2), (7, 6, 3), (9, 5, 2), (6, 2, 1), (11, 8, 4)) if group == 1 else ((7, 4, 2), (6, 5, 3)):
            out = ctypes.create_string_buffer(size)
            assert L.hm_fold_msm(cid, group, buf, sb, n, c, lgM, lgL, out) == -(-(cp.r.bit_length() + 1) // c)
            assert dec(cp, out.raw) == want, (name, group, c, lgM, lgL)


@pytest.mark.parametrize("name", CURVES)
def test_group_law_including_exceptional_cases(hostmath, name):
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("hm/ec/" + name)
    pts = [R.random_g1(cp, d) for _ in range(6)]
    seq = pts + [None, pts[0], pts[1], R.g1_neg(cp, pts[1]), pts[0]]
    buf = b"".join(R.g1_to_mont_bytes(cp, p) for p in seq)
    out = ctypes.create_string_buffer(2 * n)
    exp = None
    for p in seq:
        exp = R.g1_add(cp, exp, p)
    L.hm_g1_sum(cid, buf, None, len(seq), out)
    assert R.g1_from_mont_bytes(cp, out.raw) == exp
    L.hm_g1_tree(cid, buf, len(seq), out)
    assert R.g1_from_mont_bytes(cp, out.raw) == exp
    neg = bytes(i & 1 for i in range(len(seq)))
    exp = None
    for i, p in enumerate(seq):
        exp = R.g1_add(cp, exp, R.g1_neg(cp, p) if i & 1 else p)
    L.hm_g1_sum(cid, buf, neg, len(seq), out)
    assert R.g1_from_mont_bytes(cp, out.raw) == exp
    two = R.g1_to_mont_bytes(cp, pts[0]) * 2
    L.hm_g1_sum(cid, two, None, 2, out)
    assert R.g1_from_mont_bytes(cp, out.raw) == R.g1_add(cp, pts[0], pts[0])
    L.hm_g1_sum(cid, two, bytes([0, 1]), 2, out)
    assert R.g1_from_mont_bytes(cp, out.raw) is None
    L.hm_g1_tree(cid, two, 2, out)
    assert R.g1_from_mont_bytes(cp, out.raw) == R.g1_add(cp, pts[0], pts[0])
    qs = [R.random_g2(cp, d) for _ in range(3)]
    seq2 = qs + [None, qs[0], R.g2_neg(cp, qs[1]), qs[1]]
    buf = b"".join(R.g2_to_mont_bytes(cp, p) for p in seq2)
    out2 = ctypes.create_string_buffer(4 * n)
    exp = None
    for p in seq2:
        exp = R.g2_add(cp, exp, p)
    L.hm_g2_sum(cid, buf, None, len(seq2), out2)
    assert R.g2_from_mont_bytes(cp, out2.raw) == exp
    L.hm_g2_tree(cid, buf, len(seq2), out2)
    assert R.g2_from_mont_bytes(cp, out2.raw) == exp


@pytest.mark.parametrize("name", CURVES)
def test_miller_loop_and_final_exp(hostmath, name):
    cp = R.CURVES[name]
    T = R.tower(cp)
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("hm/pair/" + name)
    P, P2 = R.random_g1(cp, d), R.random_g1(cp, d)
    Q, Q2 = R.random_g2(cp, d), R.random_g2(cp, d)
    ml = ctypes.create_string_buffer(12 * n)
    fe = ctypes.create_string_buffer(12 * n)
    L.hm_miller(cid, R.g1_to_mont_bytes(cp, P), R.g2_to_mont_bytes(cp, Q), 1, ml)
    L.hm_fp12_op(cid, 9, ml.raw, None, fe)
    assert R.gt_from_mont_bytes(cp, fe.raw) == R.pairing(cp, P, Q)
    L.hm_miller(cid, R.g1_to_mont_bytes(cp, P) + R.g1_to_mont_bytes(cp, P2), R.g2_to_mont_bytes(cp, Q) + R.g2_to_mont_bytes(cp, Q2), 2, ml)
    L.hm_fp12_op(cid, 9, ml.raw, None, fe)
    assert R.gt_from_mont_bytes(cp, fe.raw) == T.f12_mul(R.pairing(cp, P, Q), R.pairing(cp, P2, Q2))
    L.hm_miller(cid, R.g1_to_mont_bytes(cp, None), R.g2_to_mont_bytes(cp, Q), 1, ml)
    assert R.gt_from_mont_bytes(cp, ml.raw) == T.f12_one


def _win_layout(cp, c):
    """msm_body.h: msm_win_layout -- the r.bit_length() + 1 bits spread over W windows whose widths differ by <= 1"""
    total = cp.r.bit_length() + 1
    W = (total + c - 1) // c
    base, rem = divmod(total, W)
    widths = [base + 1 if w < rem else base for w in range(W)]
    offs = [sum(widths[:w]) for w in range(W)]
    assert max(widths) <= c and max(widths) - min(widths) <= 1 and offs[-1] + widths[-1] == total
    return W, widths, offs


@pytest.mark.parametrize("name", CURVES)
def test_window_digits_reconstruct_the_scalar(hostmath, name):
    """k_digits' body: sum_w d_w 2^off(w) == s mod r, |d_w| <= 2^(width(w)-1), for plain and Montgomery inputs,
    including the all-ones windows whose carry once produced a 'minus zero' digit, over the balanced window layout
    (no sparse top window: BLS12-377 / BN254 at c = 16 get 14 + 2 resp. 15 + 1 windows of 16 / 15 bits)."""
    cp = R.CURVES[name]
    L = hostmath
    rnd = random.Random(1234)
    for c in (4, 5, 7, 10, 12, 13, 15, 16, 18, 20):
        W, widths, offs = _win_layout(cp, c)
        if name == "BLS12-381" and c == 16:
            assert widths == [16] * 16  # BASELINE configs[1]: plain 16-bit windows
        half = 1 << (c - 1)
        cases = [0, 1, cp.r - 1, cp.r - 2, (1 << c) - 1, (1 << (2 * c)) - 1, (1 << 255) % cp.r, half, half + 1, 1 << c, ((1 << c) - 1) << c]
        cases += [((1 << offs[k]) - 1) % cp.r for k in (1, 2, W // 2, W - 1)] + [((1 << (offs[k] + widths[k])) - 1) % cp.r for k in (0, W // 2)]
        cases += [((1 << (c * k)) - 1) % cp.r for k in (3, 5, 9)] + [rnd.randrange(cp.r) for _ in range(100)]

        def value(out):
            tot = 0
            for w in range(W):
                dgt = out[w]
                if dgt:
                    mag = dgt >> 1
                    assert 1 <= mag <= (1 << (widths[w] - 1)), (name, c, w)
                    tot += (-mag if dgt & 1 else mag) << offs[w]
            return tot

        for mont in (0, 1):
            for s in cases:
                enc = (s * (1 << 256) % cp.r) if mont else s
                out = (ctypes.c_uint32 * 80)()
                assert L.hm_digits(cp.curve_id, enc.to_bytes(32, "little"), mont, c, out, 80) == W
                assert value(out) == s % cp.r, (name, c, s, mont)
        for s in (cp.r, cp.r + 5, (1 << 256) - 1, 2 * cp.r + 3):  # BaseZr-style unreduced scalars
            out = (ctypes.c_uint32 * 80)()
            assert L.hm_digits(cp.curve_id, s.to_bytes(32, "little"), 0, c, out, 80) == W
            assert value(out) == s % cp.r


@pytest.mark.parametrize("name", CURVES)
def test_bucket_chunk_reduction_body(hostmath, name):
    """k_chunks' body: A = sum of 8 buckets, W0 = sum_i i * bucket_i (with infinity buckets mixed in)"""
    cp = R.CURVES[name]
    L, n = hostmath, cp.fp_bytes
    d = R.Drbg("hm/chunk/" + name)
    nch = 3
    pts = [R.random_g1(cp, d) if (i % 5) else None for i in range(8 * nch)]
    pts[9] = pts[10]  # equal neighbours -> doubling branch
    buf = b"".join(R.g1_to_mont_bytes(cp, p) for p in pts)
    oa = ctypes.create_string_buffer(2 * n * nch)
    ow = ctypes.create_string_buffer(2 * n * nch)
    assert L.hm_chunks(cp.curve_id, buf, nch, oa, ow) == 0
    for g in range(nch):
        a = w = None
        for i in range(8):
            a = R.g1_add(cp, a, pts[8 * g + i])
            w = R.g1_add(cp, w, R.g1_mul(cp, pts[8 * g + i], i) if pts[8 * g + i] is not None else None)
        assert R.g1_from_mont_bytes(cp, oa.raw[g * 2 * n : (g + 1) * 2 * n]) == a
        assert R.g1_from_mont_bytes(cp, ow.raw[g * 2 * n : (g + 1) * 2 * n]) == w


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("l_eff", [1, 2, 8])
def test_bucket_chunk_body_over_the_lane_group_forms(hostmath, name, l_eff):
    """reduce_chunk_body (msm_body.h), the one chunk loop of the reduction kernels, over the host backends of the quad and lane-pair
    additions (QuadHost, QuadHost28, PairHost: with and without the prefetch) against msm_chunk_body (form 0: the same loop over one lane) with
    xyzz_add as a point, itself checked against the oracle -- compared as affine points.  Buckets: infinities, the same point twice (acc + b and w0 + acc as
    doublings), P beside -P (acc back to infinity), and a chunk that is empty but for its last bucket."""
    cp = R.CURVES[name]
    L, n = hostmath, cp.fp_bytes
    for group, rand, neg, enc, forms in ((1, R.random_g1, R.g1_neg, R.g1_to_mont_bytes, (1, 2)),
                                         (2, R.random_g2, R.g2_neg, R.g2_to_mont_bytes, (3,))):
        d = R.Drbg("hm/chunk-forms/%s/%d" % (name, group))
        P = [rand(cp, d) for _ in range(8)]
        chunks = [[P[i % 8] if i % 3 else None for i in range(l_eff)],  # infinities mixed in
                  [P[0]] * l_eff,  # the same point in every bucket: every acc += b[i] after the first is b + b or 2b + b ...
                  [P[1], neg(cp, P[1])] * 4,  # P beside -P
                  [None] * 7 + [P[2]],  # w0 = acc after empty buckets: w0 += acc is a doubling
                  [P[3], P[3], None, neg(cp, P[3]), P[4], None, P[4], P[5]]]
        chunks = [(c * 8)[:l_eff] for c in chunks]
        buf = b"".join(enc(cp, q) for c in chunks for q in c)
        sz = 2 * n * group
        ref = [ctypes.create_string_buffer(sz * len(chunks)) for _ in range(2)]
        assert L.hm_chunks_form(cp.curve_id, group, 0, buf, len(chunks), l_eff, ref[0], ref[1]) == 0
        # the reference itself against the oracle
        add, mul, dec = (R.g1_add, R.g1_mul, R.g1_from_mont_bytes) if group == 1 else (R.g2_add, R.g2_mul, R.g2_from_mont_bytes)
        for g, c in enumerate(chunks):
            a = w = None
            for i, q in enumerate(c):
                a = add(cp, a, q)
                w = add(cp, w, mul(cp, q, i) if q is not None else None)
            assert dec(cp, ref[0].raw[g * sz : (g + 1) * sz]) == a
            assert dec(cp, ref[1].raw[g * sz : (g + 1) * sz]) == w
        for form in forms:
            out = [ctypes.create_string_buffer(sz * len(chunks)) for _ in range(2)]
            assert L.hm_chunks_form(cp.curve_id, group, form, buf, len(chunks), l_eff, out[0], out[1]) == 0
            assert out[0].raw == ref[0].raw and out[1].raw == ref[1].raw, (name, group, form, l_eff)
    assert L.hm_chunks_form(cp.curve_id, 2, 1, buf, 1, l_eff, out[0], out[1]) == -1  # no such form for that group


@pytest.mark.parametrize("T", [1, 2, 4, 8, 64])
def test_reduce_selection_lists(hostmath, T):
    """reduce_sel_index / reduce_sel_count (msm_body.h), the one place that maps element j of list sel to a chunk index:
    lists 0 and 1 partition [0, T), as do 2 and 3, split at (T + 1) / 2; list 4 + k is exactly the t with bit k set, each
    once; every list of T >= 2 has T / 2 elements; at T = 1 the second halves are empty."""
    L = hostmath
    L.hm_reduce_sel_count.restype = L.hm_reduce_sel_index.restype = ctypes.c_uint
    nb = T.bit_length() - 1
    lists = [[L.hm_reduce_sel_index(sel, j, T) for j in range(L.hm_reduce_sel_count(sel, T))] for sel in range(4 + nb)]
    half = (T + 1) // 2
    for a, b in ((0, 1), (2, 3)):
        assert lists[a] == list(range(half)) and lists[b] == list(range(half, T))
    for k in range(nb):
        assert lists[4 + k] == [t for t in range(T) if (t >> k) & 1]
    if T >= 2:
        assert all(len(l) == T // 2 for l in lists)
    else:
        assert [len(l) for l in lists] == [1, 0, 1, 0]


@pytest.mark.parametrize("name", list(R.CURVES))
def test_g1_wire_codec(hostmath, name):
    """csrc/codec.h (sqrt incl. Tonelli-Shanks for BLS12-377, flag handling, subgroup check) vs the oracle's
    restatement of gnark's SetBytes / Bytes / RawBytes."""
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/codec/" + name)
    pts = [R.random_g1(cp, d) for _ in range(6)] + [None, cp.g1]
    for P in pts:
        for comp, enc in ((1, R.g1_wire_compressed), (0, R.g1_wire_uncompressed)):
            w = enc(cp, P)
            out = ctypes.create_string_buffer(2 * n)
            assert L.hm_g1_decode(cid, w, comp, 1, out) == 0
            assert out.raw == R.g1_to_mont_bytes(cp, P)
            back = ctypes.create_string_buffer(len(w))
            L.hm_g1_encode(cid, out.raw, comp, back)
            assert back.raw == w
    bad = []
    x = 1
    while len(bad) < 3:
        x += 1
        if R.fp_sqrt((x**3 + cp.b) % cp.p, cp.p) is None:
            w = bytearray(x.to_bytes(n, "big"))
            w[0] |= 0x80
            bad.append(bytes(w))
    w = bytearray(cp.p.to_bytes(n, "big"))
    w[0] |= 0x80
    bad.append(bytes(w))
    w = bytearray(R.g1_wire_compressed(cp, None))
    w[5] = 1
    bad.append(bytes(w))
    if cp.family == "BLS12":
        x = 2
        while True:
            y = R.fp_sqrt((x**3 + cp.b) % cp.p, cp.p)
            if y is not None and R.g1_mul_unreduced(cp, (x, y), cp.r) is not None:
                break
            x += 1
        bad.append(R.g1_wire_compressed(cp, (x, y)))
        out = ctypes.create_string_buffer(2 * n)
        assert L.hm_g1_decode(cid, bad[-1], 1, 0, out) == 0  # accepted when the subgroup check is off
        assert out.raw == R.g1_to_mont_bytes(cp, (x, y))
    for w in bad:
        out = ctypes.create_string_buffer(2 * n)
        want = R.g1_from_wire(cp, w)[1]
        assert want != 0
        assert L.hm_g1_decode(cid, w, 1, 1, out) == want
        assert out.raw == bytes(2 * n)


def _g2_out_of_subgroup(cp):
    """a point of E'(Fp2) outside the r-torsion (the twist's cofactor is huge, so the first point found serves)"""
    Q = R._g2_some_point(cp, 3)
    assert R.g2_mul_unreduced(cp, Q, cp.r) is not None
    return Q


@pytest.mark.parametrize("name", list(R.CURVES))
def test_g2_wire_codec(hostmath, name):
    """csrc/codec.h G2 half (Fp2 square root by the norm, E2 'largest' rule, A1-first byte order, [r]Q test)."""
    cp = R.CURVES[name]
    T = R.tower(cp)
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/codec2/" + name)
    g2 = R.g2_generator(cp)
    pts = [R.random_g2(cp, d) for _ in range(3)] + [None, g2, R.g2_neg(cp, g2)]
    for Q in pts:
        for comp, enc in ((1, R.g2_wire_compressed), (0, R.g2_wire_uncompressed)):
            w = enc(cp, Q)
            assert R.g2_from_wire(cp, w) == (Q, 0)
            out = ctypes.create_string_buffer(4 * n)
            assert L.hm_g2_decode(cid, w, comp, 1, out) == 0
            assert out.raw == R.g2_to_mont_bytes(cp, Q)
            back = ctypes.create_string_buffer(len(w))
            L.hm_g2_encode(cid, out.raw, comp, back)
            assert back.raw == w
    bad = []
    k = 1
    while len(bad) < 3:  # x^3 + b' not a square in Fp2; one of them with A1 = 0
        k += 1
        x = (k, 0) if len(bad) == 0 else (k, 1)
        if T.f2_sqrt(T.f2_add(T.f2_mul(T.f2_sqr(x), x), R.twist_b(cp))) is None:
            w = bytearray(x[1].to_bytes(n, "big") + x[0].to_bytes(n, "big"))
            w[0] |= 0x80
            bad.append(bytes(w))
    w = bytearray((1).to_bytes(n, "big") + cp.p.to_bytes(n, "big"))  # X.A0 >= p
    w[0] |= 0x80
    bad.append(bytes(w))
    w = bytearray(R.g2_wire_compressed(cp, None))
    w[n + 3] = 1
    bad.append(bytes(w))
    Qx = _g2_out_of_subgroup(cp)
    bad.append(R.g2_wire_compressed(cp, Qx))
    out = ctypes.create_string_buffer(4 * n)
    assert L.hm_g2_decode(cid, bad[-1], 1, 0, out) == 0
    assert out.raw == R.g2_to_mont_bytes(cp, Qx)
    for w in bad:
        out = ctypes.create_string_buffer(4 * n)
        want = R.g2_from_wire(cp, w)[1]
        assert want != 0
        assert L.hm_g2_decode(cid, w, 1, 1, out) == want
        assert out.raw == bytes(4 * n)
    # purely real / purely imaginary square roots (a1 = 0 branch of fp2_sqrt), through y^2 = x^3 + b' is hard to hit:
    # exercise them through points whose y happens to need the "largest" flip instead
    for Q in pts[:3]:
        w = bytearray(R.g2_wire_compressed(cp, Q))
        w[0] ^= 0x20 if cp.family == "BLS12" else 0x40
        out = ctypes.create_string_buffer(4 * n)
        assert L.hm_g2_decode(cid, bytes(w), 1, 1, out) == 0
        assert out.raw == R.g2_to_mont_bytes(cp, R.g2_neg(cp, Q))


@pytest.mark.parametrize("name", list(R.CURVES))
def test_fp2_sqrt_all_branches(hostmath, name):
    cp = R.CURVES[name]
    T = R.tower(cp)
    L, cid = hostmath, cp.curve_id

    def mont2(a):
        return R.fp_to_mont_bytes(cp, a[0]) + R.fp_to_mont_bytes(cp, a[1])

    d = R.Drbg("host/fp2sqrt/" + name)
    nonres = next(v for v in range(2, 50) if R.fp_sqrt(v, cp.p) is None)
    cases = [(4, 0), (nonres, 0), (0, 0), (0, 1), (cp.p - 1, 0)]  # real square, real non-residue, zero, pure imaginary
    cases += [(d.below(cp.p), d.below(cp.p)) for _ in range(12)]
    squares = 0
    for a in cases:
        out = ctypes.create_string_buffer(2 * cp.fp_bytes)
        rc = L.hm_fp2_op(cid, 4, mont2(a), None, out)
        want = T.f2_sqrt(a)
        assert rc == (1 if want is None else 0), a
        if want is not None:
            squares += 1
            r = (R.fp_from_mont_bytes(cp, out.raw[: cp.fp_bytes]), R.fp_from_mont_bytes(cp, out.raw[cp.fp_bytes :]))
            assert T.f2_sqr(r) == (a[0] % cp.p, a[1] % cp.p)  # either root is valid; the codec fixes the sign afterwards
    assert 5 <= squares < len(cases)


@pytest.mark.parametrize("name", list(R.CURVES))
def test_fp28_carry_free_form(hostmath, name):
    """csrc/fp28.h: conversions, product / square / dual product, lazy sums at the documented weight limits and
    the exact zero test, against Python integers."""
    cp = R.CURVES[name]
    L, cid, p = hostmath, cp.curve_id, cp.p
    d = R.Drbg("host/fp28/" + name)
    mb = lambda v: R.fp_to_mont_bytes(cp, v % p)

    def run(op, vals):
        out = ctypes.create_string_buffer(cp.fp_bytes)
        args = [mb(v) for v in vals] + [None] * (4 - len(vals))
        assert L.hm_fp28_op(cid, op, *args, out) == 0
        return out.raw

    edge = [0, 1, p - 1, p - 2, (p - 1) // 2, 2, (1 << 28) - 1, 1 << 28, (1 << (cp.fp_bytes * 8 - 8)) % p]
    rnd = [d.below(p) for _ in range(24)]
    for a in edge + rnd[:8]:
        assert run(0, [a]) == mb(a)
        assert run(2, [a]) == mb(a * a)
    vals = edge + rnd
    for i in range(0, len(vals) - 3):
        a, b, c, e = vals[i : i + 4]
        assert run(1, [a, b]) == mb(a * b)
        assert run(3, [a, b, c, e]) == mb(a * b + c * e)
        assert run(5, [a, b, c, e]) == mb((a + b) * (c - e))
        assert run(6, [a, b, c, e]) == mb((a - b - 2 * c) * e)
        assert run(7, [a, b]) == mb((a - b) ** 2)
    zt = ctypes.create_string_buffer(cp.fp_bytes)
    for a, b in [(5, 5), (0, 0), (p - 1, p - 1), (rnd[0], rnd[0]), (rnd[0], rnd[1]), (1, 0), (0, p - 1)]:
        assert L.hm_fp28_op(cid, 4, mb(a), mb(b), None, None, zt) == 0
        assert int.from_bytes(zt.raw[:4], "little") == (1 if (a - b) % p == 0 else 0)


@pytest.mark.parametrize("name", list(R.CURVES))
def test_madd28_bucket_accumulation(hostmath, name):
    """ec28.h: a bucket's running sum in the carry-free form equals the oracle's, including the exceptional
    cases (P + P, P - P, infinity inputs, restart after cancelling to infinity)."""
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/madd28/" + name)
    P = [R.random_g1(cp, d) for _ in range(6)]
    cases = [
        [(P[0], 0)],
        [(P[0], 1)],
        [(P[i], i & 1) for i in range(6)],
        [(P[0], 0), (P[0], 0), (P[1], 0)],            # doubling inside the chain
        [(P[0], 0), (P[0], 1), (P[1], 1), (P[2], 0)],  # cancels to infinity, then restarts
        [(None, 0), (P[3], 0), (None, 1), (P[3], 0), (P[3], 0)],
        [(P[0], 0), (P[1], 0), (R.g1_add(cp, P[0], P[1]), 1)],  # ends at infinity
        [(P[i % 6], (i * 7) & 1) for i in range(40)],
    ]
    for seq in cases:
        pts = b"".join(R.g1_to_mont_bytes(cp, q) for q, _ in seq)
        neg = bytes(s for _, s in seq)
        want = None
        for q, s in seq:
            want = R.g1_add(cp, want, R.g1_neg(cp, q) if s else q)
        out = ctypes.create_string_buffer(2 * n)
        assert L.hm_madd28_chain(cid, pts, neg, len(seq), out) == 0
        assert out.raw == R.g1_to_mont_bytes(cp, want)


@pytest.mark.parametrize("name", list(R.CURVES))
def test_quad_lane_xyzz_add(hostmath, name):
    """ec_quad.h: the four-rounds-of-one-multiplication schedule of XYZZ + XYZZ (host emulation of the DPP
    permutes) equals the oracle, including doubling, cancellation and infinity operands."""
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/quad/" + name)
    P = [R.random_g1(cp, d) for _ in range(5)]
    neg = lambda q: R.g1_neg(cp, q)
    cases = [
        [P[0]],
        [P[0], P[1], P[2], P[3], P[4]],
        [P[0], P[0]],                      # doubling (different z on both sides)
        [P[0], P[1], neg(R.g1_add(cp, P[0], P[1])), P[2]],  # hits infinity, then restarts
        [None, P[0], None, P[1]],
        [P[2], neg(P[2])],
        [P[i % 5] for i in range(23)],
    ]
    if name == "BLS12-377":  # y^2 = x^3 + 1 has a point of order two, (-1, 0): doubling it must give infinity
        T2 = (cp.p - 1, 0)
        cases += [[T2, T2], [P[0], T2, T2, P[1]], [T2, P[0], T2]]
    for seq in cases:
        pts = b"".join(R.g1_to_mont_bytes(cp, q) for q in seq)
        zs = b"".join(R.fp_to_mont_bytes(cp, 1 + d.below(cp.p - 1)) for _ in seq)
        want = None
        for q in seq:
            want = R.g1_add(cp, want, q)
        out = ctypes.create_string_buffer(2 * n)
        assert L.hm_quad_chain(cid, pts, zs, len(seq), out) == 0
        assert out.raw == R.g1_to_mont_bytes(cp, want)
        out = ctypes.create_string_buffer(2 * n)  # the carry-free form of the same schedule (ec_quad28.h)
        assert L.hm_quad28_chain(cid, pts, zs, len(seq), out) == 0
        assert out.raw == R.g1_to_mont_bytes(cp, want)


@pytest.mark.parametrize("name", ["BN254", "BLS12-381", "BLS12-377"])
def test_madd28_lane_pair_g2_accumulation(hostmath, name):
    """ec28_lp.h (G2, u^2 = -1 curves): bucket sums in the carry-free lane-pair form, host emulation of the pair
    exchange, against the oracle -- including doubling, cancellation, infinity inputs."""
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/madd28lp/" + name)
    P = [R.random_g2(cp, d) for _ in range(5)]
    cases = [
        [(P[0], 0)],
        [(P[0], 1)],
        [(P[i], i & 1) for i in range(5)],
        [(P[0], 0), (P[0], 0), (P[1], 0)],
        [(P[0], 0), (P[0], 1), (P[1], 1), (P[2], 0)],
        [(None, 0), (P[3], 0), (None, 1), (P[3], 0), (P[3], 0)],
        [(P[0], 0), (P[1], 0), (R.g2_add(cp, P[0], P[1]), 1)],
        [(P[i % 5], (i * 7) & 1) for i in range(24)],
    ]
    for seq in cases:
        pts = b"".join(R.g2_to_mont_bytes(cp, q) for q, _ in seq)
        neg = bytes(s for _, s in seq)
        want = None
        for q, s in seq:
            want = R.g2_add(cp, want, R.g2_neg(cp, q) if s else q)
        out = ctypes.create_string_buffer(4 * n)
        assert L.hm_madd28_lp_chain(cid, pts, neg, len(seq), out) == 0
        assert out.raw == R.g2_to_mont_bytes(cp, want)
        # ec28_kc.h: the pair split by coordinate, one-lane Karatsuba Fp2 products; also checks (inside) that the
        # bucket state equals the component split's bit for bit after every addition
        if cp.beta == -1:
            out = ctypes.create_string_buffer(4 * n)
            assert L.hm_madd28_kc_chain(cid, pts, neg, len(seq), out) == 0
            assert out.raw == R.g2_to_mont_bytes(cp, want)
    # the full addition of the carry-free G2 reduction (xyzz28_lp_add): operands with random Z, doubling, cancellation
    for seq in cases:
        pts = b"".join(R.g2_to_mont_bytes(cp, R.g2_neg(cp, q) if s else q) for q, s in seq)
        zs = b"".join(R.fp_to_mont_bytes(cp, 1 + d.below(cp.p - 1)) + R.fp_to_mont_bytes(cp, d.below(cp.p)) for _ in seq)
        want = None
        for q, s in seq:
            want = R.g2_add(cp, want, R.g2_neg(cp, q) if s else q)
        out = ctypes.create_string_buffer(4 * n)
        assert L.hm_add28_lp_chain(cid, pts, zs, len(seq), out) == 0
        assert out.raw == R.g2_to_mont_bytes(cp, want)


def test_ed28_twisted_edwards_g1_accumulation(hostmath):
    """ed28.h (BLS12-377 G1): bucket sums in extended twisted Edwards coordinates over the carry-free form -- the batched
    Weierstrass -> Edwards conversion (one shared inversion per four points, infinity inputs), the 7-product mixed
    addition incl. doubling (P + P), cancellation (P - P), negated inputs, the full addition and the way back to XYZZ --
    against the oracle's Weierstrass sums; also the oracle's own statement of the map."""
    cp = R.CURVES["BLS12-377"]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/ed28")
    P = [R.g1_mul(cp, cp.g1, 1 + d.below(cp.r - 1)) for _ in range(6)]
    for q in P[:3]:  # the oracle's map is a group isomorphism on G1
        e = R.g1_to_edwards(cp, q)
        assert R.edwards_to_g1(cp, e) == q
        assert R.edwards_to_g1(cp, R.edwards_add(cp, e, R.g1_to_edwards(cp, P[3]))) == R.g1_add(cp, q, P[3])
    cases = [
        [(P[0], 0)],
        [(P[0], 1)],
        [(P[i], i & 1) for i in range(6)],
        [(P[0], 0), (P[0], 0), (P[1], 0)],
        [(P[0], 0), (P[0], 1)],
        [(P[0], 0), (P[0], 1), (P[1], 1), (P[2], 0)],
        [(None, 0), (P[3], 0), (None, 1), (P[3], 0), (P[3], 0)],
        [(None, 0), (None, 1)],
        [(P[0], 0), (P[1], 0), (R.g1_add(cp, P[0], P[1]), 1)],
        [(P[i % 6], (i * 7) & 1) for i in range(37)],
    ]
    for seq in cases:
        pts = b"".join(R.g1_to_mont_bytes(cp, q) for q, _ in seq)
        neg = bytes(s for _, s in seq)
        want = None
        for q, s in seq:
            want = R.g1_add(cp, want, R.g1_neg(cp, q) if s else q)
        for mode in (0, 1, 2, 3):  # mixed additions, full additions, the quad-lane schedule, that with doublings
            out = ctypes.create_string_buffer(2 * n)
            assert L.hm_ed28_chain(cid, pts, neg, len(seq), mode, out) == 0
            assert out.raw == R.g1_to_mont_bytes(cp, want), (mode, len(seq))
    out = ctypes.create_string_buffer(2 * R.CURVES["BLS12-381"].fp_bytes)
    assert L.hm_ed28_chain(R.CURVES["BLS12-381"].curve_id, b"", b"", 0, 0, out) == -2  # no Edwards model of that curve


@pytest.mark.parametrize("name", list(R.CURVES))
def test_divsteps_inversion(hostmath, name):
    """modinv.h (Bernstein-Yang divsteps, fixed iteration count) against Python's pow(x, -1, p): edge values, values
    whose gcd chains are long (Fibonacci-like neighbours), and random ones; 0 maps to 0 as with Fermat."""
    cp = R.CURVES[name]
    L, cid, p = hostmath, cp.curve_id, cp.p
    d = R.Drbg("host/modinv/" + name)
    vals = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 30, (1 << 30) - 1, 1 << 60, (1 << (p.bit_length() - 1)),
            (1 << (p.bit_length() - 1)) - 1, cp.R % p, pow(cp.R, -1, p)]
    a, b = 1, 2
    while b < p:  # consecutive Fibonacci numbers: the classical worst case of Euclid-type chains
        a, b = b, a + b
    vals += [a, b - a, p - a]
    vals += [d.below(p) for _ in range(200)]
    for x in vals:
        out = ctypes.create_string_buffer(cp.fp_bytes)
        assert L.hm_fp_op(cid, 9, R.fp_to_mont_bytes(cp, x), None, out) == 0
        want = pow(x, -1, p) if x % p else 0
        assert out.raw == R.fp_to_mont_bytes(cp, want), (name, x)


@pytest.mark.parametrize("name", ["BLS12-381", "BLS12-377"])
def test_g1_subgroup_test_by_endomorphism(hostmath, name):
    """codec.h g1_in_subgroup_endo (phi(P) = [-x^2]P) must agree with the plain [r]P ladder on every kind of curve
    point: r-torsion points, random curve points (cofactor components), points of each small prime order dividing the
    cofactor, and sums subgroup + small-order."""
    from math import gcd

    cp = R.CURVES[name]
    L, cid, n, p = hostmath, cp.curve_id, cp.fp_bytes, cp.p
    d = R.Drbg("host/endo/" + name)
    order = p + 1 - (cp.x + 1)  # #E(Fp) for BLS12: t = x + 1
    h = order // cp.r
    assert h * cp.r == order

    def curve_point():
        while True:
            x = d.below(p)
            y = R.fp_sqrt((x * x * x + cp.b) % p, p)
            if y is not None:
                return (x, y)

    # small prime factors of the cofactor (trial division is enough for these h)
    fac, m, q = [], h, 2
    while q * q <= m and q < 1 << 22:
        if m % q == 0:
            fac.append(q)
            while m % q == 0:
                m //= q
        q += 1
    if m > 1:
        fac.append(m)
    pts = [R.random_g1(cp, d) for _ in range(3)] + [cp.g1]
    bad = []
    for _ in range(4):
        bad.append(curve_point())
    for ell in fac:  # a point of exact order ell
        for _ in range(20):
            T = R.g1_mul_unreduced(cp, curve_point(), order // ell)
            if T is not None:
                bad.append(T)
                bad.append(R.g1_add(cp, T, pts[0]))  # subgroup point + small-order point
                break
    assert len(bad) >= 6
    for P, want in [(q_, True) for q_ in pts] + [(q_, R.g1_mul_unreduced(cp, q_, cp.r) is None) for q_ in bad]:
        w = R.g1_wire_uncompressed(cp, P)
        got = {}
        for mode in (1, 2):
            out = ctypes.create_string_buffer(2 * n)
            st = L.hm_g1_decode(cid, w, 0, mode, out)
            assert st in (0, 3)
            got[mode] = st == 0
        assert got[1] == got[2] == want, (name, P)


@pytest.mark.parametrize("name", ["BLS12-381", "BLS12-377", "BN254"])
def test_g2_subgroup_test_by_psi(hostmath, name):
    """codec.h g2_in_subgroup_psi (psi(Q) = [x]Q) agrees with the plain [r]Q ladder on r-torsion points, random twist
    points, points of small prime order dividing the G2 cofactor, and sums of the two kinds."""
    cp = R.CURVES[name]
    L, cid, n = hostmath, cp.curve_id, cp.fp_bytes
    d = R.Drbg("host/psi/" + name)
    order = R.g2_order(cp)
    h2 = order // cp.r
    fac, m, q = [], h2, 2
    while q < 1 << 16 and m > 1:
        if m % q == 0:
            fac.append(q)
            while m % q == 0:
                m //= q
        q += 1
    good = [R.random_g2(cp, d) for _ in range(2)] + [R.g2_generator(cp)]
    bad = [R._g2_some_point(cp, 5 + 7 * i) for i in range(3)]
    for ell in fac[:4]:
        for i in range(10):
            T = R.g2_mul_unreduced(cp, R._g2_some_point(cp, 100 + 13 * i + ell), order // ell)
            if T is not None:
                bad.append(T)
                bad.append(R.g2_add(cp, T, good[0]))
                break
    for Q, want in [(q_, True) for q_ in good] + [(q_, R.g2_mul_unreduced(cp, q_, cp.r) is None) for q_ in bad]:
        w = R.g2_wire_uncompressed(cp, Q)
        got = {}
        for mode in (1, 2):
            out = ctypes.create_string_buffer(4 * n)
            st = L.hm_g2_decode(cid, w, 0, mode, out)
            assert st in (0, 3)
            got[mode] = st == 0
        assert got[1] == got[2] == want, (name, Q)
    assert any(not w_ for _, w_ in [(q_, R.g2_mul_unreduced(cp, q_, cp.r) is None) for q_ in bad])


# ---- carry-free lane-pair element of the BLS12-381 pairing kernels (fp2_lanes28.h) through its host model ---------
def test_lp28_tower_ops_and_weight_budget(hostmath):
    """Every Fp12-level operation of the pairing on the carry-free element: the host model (Fp2H28: both lanes of a
    pair + the weight and value bound of every value) runs the SAME tower templates as the kernels, aborts if any
    product / square / stored value exceeds its budget, and returns the largest weight left in the result (the
    formulas promise normalized results).  Values against the oracle."""
    cp = R.CURVES["BLS12-381"]
    T = R.tower(cp)
    L = hostmath
    d = R.Drbg("hm/lp28/ops")
    rf = lambda: tuple((d.below(cp.p), d.below(cp.p)) for _ in range(6))  # noqa: E731
    gb = lambda f: R.gt_to_mont_bytes(cp, f)  # noqa: E731
    out = ctypes.create_string_buffer(576)
    for _ in range(2):
        f, g = rf(), rf()
        c = T.f12_mul(T.f12_conj(f), T.f12_inv(f))
        c = T.f12_mul(T.f12_frob(c, 2), c)  # cyclotomic subgroup element
        cases = [(0, f, T.f12_mul(f, g)), (1, f, T.f12_sqr(f)), (10, f, T.f12_mul(f, g)), (11, f, T.f12_sqr(f)), (2, f, T.f12_inv(f)),
                 (3, f, T.f12_frob(f, 1)), (4, f, T.f12_frob(f, 2)), (5, f, T.f12_frob(f, 3)), (7, f, T.f12_conj(f)),
                 (6, c, T.f12_sqr(c)), (8, c, T.f12_pow(c, cp.x)), (9, f, R.final_exp(cp, f))]
        for op, a, exp in cases:
            assert L.hm_lp28_fp12_op(op, gb(a), gb(g), out) == 1, op
            assert R.gt_from_mont_bytes(cp, out.raw) == exp, op
    # chains of compressed cyclotomic squarings: the linear terms must not let the value grow (fp2_reduce)
    for n in (1, 2, 17, 63):
        assert L.hm_lp28_fp12_op(12, gb(c), bytes([n]) + bytes(575), out) == 1
        exp = c
        for _ in range(n):
            exp = T.f12_sqr(exp)
        assert R.gt_from_mont_bytes(cp, out.raw) == exp, n
    # edge values: 1, and an element with B = C = 0 in the compressed form
    one = tuple([(1, 0)] + [(0, 0)] * 5)
    assert L.hm_lp28_fp12_op(8, gb(one), None, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one
    assert L.hm_lp28_fp12_op(9, gb(one), None, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one


def test_lp28_pairing_matches_oracle(hostmath):
    """Whole pairings through the host model: Miller loop + final exponentiation (one pair, two pairs sharing the
    squarings, a pair with a point at infinity) against oracle/pyref.py."""
    cp = R.CURVES["BLS12-381"]
    L = hostmath
    d = R.Drbg("hm/lp28/pairing")
    out = ctypes.create_string_buffer(576)
    P, Q = R.random_g1(cp, d), R.random_g2(cp, d)
    P2, Q2 = R.random_g1(cp, d), R.random_g2(cp, d)
    g1 = R.g1_to_mont_bytes(cp, P) + R.g1_to_mont_bytes(cp, P2)
    g2 = R.g2_to_mont_bytes(cp, Q) + R.g2_to_mont_bytes(cp, Q2)
    assert L.hm_lp28_pairing(g1, g2, 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)
    assert L.hm_lp28_pairing(g1, g2, 2, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.final_exp(cp, R.miller_loop(cp, [(P, Q), (P2, Q2)]))
    # generator pairing = the golden GenGt; infinity on either side gives 1
    g = load_golden("BLS12-381")
    c0 = g["pairing"][0]
    assert L.hm_lp28_pairing(bytes.fromhex(c0["g1"]), bytes.fromhex(c0["g2"]), 1, 1, out) == 1
    assert out.raw.hex() == c0["fexp"]
    one = tuple([(1, 0)] + [(0, 0)] * 5)
    assert L.hm_lp28_pairing(bytes(96), R.g2_to_mont_bytes(cp, Q), 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == one
    assert L.hm_lp28_pairing(R.g1_to_mont_bytes(cp, P) + bytes(96), R.g2_to_mont_bytes(cp, Q) + R.g2_to_mont_bytes(cp, Q2), 2, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)


def test_fp28_reduce_range(hostmath):
    """fp28_reduce: value -> value - round(value / p) p from a float estimate of the top limb; the result must be the
    same residue with |result| < 0.6 p for every storable input (weight <= 8, |value| up to ~600 p)."""
    cp = R.CURVES["BLS12-381"]
    L = hostmath
    d = R.Drbg("hm/reduce")
    p = cp.p
    out = (ctypes.c_int32 * 14)()
    for trial in range(400):
        scale = [1, 2, 7, 50, 300, 600][trial % 6]
        v = (d.below(2 * scale * p) - scale * p)
        # spread over 14 signed limbs of up to 3 extra bits
        limbs, rest = [], v
        for i in range(13):
            l = rest & ((1 << 28) - 1)
            if trial % 3 == 1:
                l += (d.below(15) - 7) << 28  # un-normalized: weight up to 8
            limbs.append(l)
            rest = (rest - l) >> 28
        limbs.append(rest)
        assert sum(l << (28 * i) for i, l in enumerate(limbs)) == v
        arr = (ctypes.c_int32 * 14)(*limbs)
        assert L.hm_fp28_reduce(1, arr, out) == 0
        got = sum(int(out[i]) << (28 * i) for i in range(14))
        assert (got - v) % p == 0 and abs(got) < 0.6 * p, (trial, v / p, got / p)
        assert all(0 <= int(out[i]) < (1 << 28) for i in range(13))


@pytest.mark.parametrize("name", ["BLS12-377", "BN254"])
def test_lp28_other_curves_tower_and_pairing(hostmath, name):
    """The carry-free lane-pair element on BLS12-377 (u^2 = -5, xi = u, D-twist) and BN254 (10 limbs, xi = 9 + u, the BN
    loop and final exponentiation): every Fp12-level operation, the compressed squaring chains, the final exponentiation and
    whole pairings (one pair, two pairs, Miller loop alone, infinity) through the host model -- which aborts on any weight or
    value-bound violation -- against the oracle.  With u^2 = -5 the c0 lane's dual product weighs (1 + 5) w_a w_b: fp2_mul
    carry-propagates both operands, fp2_sqr is the two-term form."""
    cp = R.CURVES[name]
    T = R.tower(cp)
    L, cid = hostmath, cp.curve_id
    d = R.Drbg("hm/lp28/" + name)
    rf = lambda: tuple((d.below(cp.p), d.below(cp.p)) for _ in range(6))  # noqa: E731
    gb = lambda f: R.gt_to_mont_bytes(cp, f)  # noqa: E731
    nb, g1n, g2n = 12 * cp.fp_bytes, 2 * cp.fp_bytes, 4 * cp.fp_bytes
    out = ctypes.create_string_buffer(nb)
    f, g = rf(), rf()
    c = T.f12_mul(T.f12_conj(f), T.f12_inv(f))
    c = T.f12_mul(T.f12_frob(c, 2), c)  # cyclotomic subgroup element
    cases = [(0, f, T.f12_mul(f, g)), (1, f, T.f12_sqr(f)), (10, f, T.f12_mul(f, g)), (11, f, T.f12_sqr(f)), (2, f, T.f12_inv(f)),
             (3, f, T.f12_frob(f, 1)), (4, f, T.f12_frob(f, 2)), (5, f, T.f12_frob(f, 3)), (7, f, T.f12_conj(f)),
             (6, c, T.f12_sqr(c)), (8, c, T.f12_pow(c, abs(cp.x))), (9, f, R.final_exp(cp, f))]
    for op, a, exp in cases:
        assert L.hm_lp28c_fp12_op(cid, op, gb(a), gb(g), out) == 1, op
        assert R.gt_from_mont_bytes(cp, out.raw) == exp, op
    for n in (1, 2, 17, 63):  # chains of compressed cyclotomic squarings
        assert L.hm_lp28c_fp12_op(cid, 12, gb(c), bytes([n]) + bytes(nb - 1), out) == 1
        exp = c
        for _ in range(n):
            exp = T.f12_sqr(exp)
        assert R.gt_from_mont_bytes(cp, out.raw) == exp, n
    P, Q = R.random_g1(cp, d), R.random_g2(cp, d)
    P2, Q2 = R.random_g1(cp, d), R.random_g2(cp, d)
    g1 = R.g1_to_mont_bytes(cp, P) + R.g1_to_mont_bytes(cp, P2)
    g2 = R.g2_to_mont_bytes(cp, Q) + R.g2_to_mont_bytes(cp, Q2)
    assert L.hm_lp28c_pairing(cid, g1, g2, 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)
    assert L.hm_lp28c_pairing(cid, g1, g2, 2, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.final_exp(cp, R.miller_loop(cp, [(P, Q), (P2, Q2)]))
    assert L.hm_lp28c_pairing(cid, g1, g2, 1, 0, out) == 1
    assert R.final_exp(cp, R.gt_from_mont_bytes(cp, out.raw)) == R.pairing(cp, P, Q)
    one = tuple([(1, 0)] + [(0, 0)] * 5)
    assert L.hm_lp28c_pairing(cid, bytes(g1n), R.g2_to_mont_bytes(cp, Q), 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == one
    assert L.hm_lp28c_pairing(cid, R.g1_to_mont_bytes(cp, P), bytes(g2n), 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == one


def test_q28_tower_ops_and_weight_budget(hostmath):
    """pairing_quad.h: every Fp12-level operation of the quad-lane pairing through its host model (Fp2Q28H: the four
    lanes of a quad, pair A = the c0 half and pair B = the c1 half of an Fp12, with the weight / value-bound checks of
    the lane-pair model and a check that no branch depends on a value that differs between the pairs)."""
    cp = R.CURVES["BLS12-381"]
    T = R.tower(cp)
    L = hostmath
    d = R.Drbg("hm/q28/ops")
    rf = lambda: tuple((d.below(cp.p), d.below(cp.p)) for _ in range(6))  # noqa: E731
    gb = lambda f: R.gt_to_mont_bytes(cp, f)  # noqa: E731
    out = ctypes.create_string_buffer(576)
    for _ in range(2):
        f, g = rf(), rf()
        c = T.f12_mul(T.f12_conj(f), T.f12_inv(f))
        c = T.f12_mul(T.f12_frob(c, 2), c)  # cyclotomic subgroup element
        cases = [(0, f, T.f12_mul(f, g)), (1, f, T.f12_sqr(f)), (10, f, T.f12_mul(f, g)), (11, f, T.f12_sqr(f)), (2, f, T.f12_inv(f)),
                 (3, f, T.f12_frob(f, 1)), (4, f, T.f12_frob(f, 2)), (5, f, T.f12_frob(f, 3)), (7, f, T.f12_conj(f)),
                 (8, c, T.f12_pow(c, cp.x)), (9, f, R.final_exp(cp, f))]
        for op, a, exp in cases:
            assert L.hm_q28_fp12_op(op, gb(a), gb(g), out) == 1, op
            assert R.gt_from_mont_bytes(cp, out.raw) == exp, op
    for n in (1, 2, 17, 63):
        assert L.hm_q28_fp12_op(12, gb(c), bytes([n]) + bytes(575), out) == 1
        exp = c
        for _ in range(n):
            exp = T.f12_sqr(exp)
        assert R.gt_from_mont_bytes(cp, out.raw) == exp, n
    one = tuple([(1, 0)] + [(0, 0)] * 5)
    assert L.hm_q28_fp12_op(8, gb(one), None, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one
    assert L.hm_q28_fp12_op(9, gb(one), None, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one


def test_q28_pairing_matches_oracle(hostmath):
    """Whole pairings through the quad-lane host model: Miller loop alone (compared after the oracle's final
    exponentiation), fused pairing, two pairs sharing the squarings (Pairing2), the golden generator pairing, infinity
    on either side."""
    cp = R.CURVES["BLS12-381"]
    L = hostmath
    d = R.Drbg("hm/q28/pairing")
    out = ctypes.create_string_buffer(576)
    P, Q = R.random_g1(cp, d), R.random_g2(cp, d)
    P2, Q2 = R.random_g1(cp, d), R.random_g2(cp, d)
    g1, g2 = R.g1_to_mont_bytes(cp, P), R.g2_to_mont_bytes(cp, Q)
    assert L.hm_q28_pairing(g1, g2, 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)
    assert L.hm_q28_pairing(g1, g2, 1, 0, out) == 1
    assert R.final_exp(cp, R.gt_from_mont_bytes(cp, out.raw)) == R.pairing(cp, P, Q)
    assert L.hm_q28_pairing(g1 + R.g1_to_mont_bytes(cp, P2), g2 + R.g2_to_mont_bytes(cp, Q2), 2, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.final_exp(cp, R.miller_loop(cp, [(P, Q), (P2, Q2)]))
    assert L.hm_q28_pairing(g1 + bytes(96), g2 + R.g2_to_mont_bytes(cp, Q2), 2, 1, out) == 1  # second pair not live
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)
    g = load_golden("BLS12-381")
    c0 = g["pairing"][0]
    assert L.hm_q28_pairing(bytes.fromhex(c0["g1"]), bytes.fromhex(c0["g2"]), 1, 1, out) == 1
    assert out.raw.hex() == c0["fexp"]
    one = tuple([(1, 0)] + [(0, 0)] * 5)
    assert L.hm_q28_pairing(bytes(96), g2, 1, 1, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one
    assert L.hm_q28_pairing(g1, bytes(192), 1, 1, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one


@pytest.mark.parametrize("name", ["BLS12-377", "BN254"])
def test_q28_other_curves_tower_and_pairing(hostmath, name):
    """Round 4: the quad-lane pairing on BLS12-377 (pairing_quad.h: the D-twist line product fp12q_mul_by_034, the doubling
    step with 3 b' as a constant, u^2 = -5 in every Fp2 product of both pairs) and on BN254 (10 limbs, xi = 9 + u, the two
    Frobenius lines after the loop, the Fuentes-Castaneda hard part on plain squarings) through the quad host model --
    every weight and value budget checked, no branch on a value that differs between the pairs: the Fp12 operations,
    squaring chains, the sparse line product, final exponentiation, pairings with one and two pairs, infinities."""
    cp = R.CURVES[name]
    cid = cp.curve_id
    T = R.tower(cp)
    L = hostmath
    d = R.Drbg("hm/q28/" + name)
    n = cp.fp_bytes
    rf = lambda: tuple((d.below(cp.p), d.below(cp.p)) for _ in range(6))  # noqa: E731
    gb = lambda f: R.gt_to_mont_bytes(cp, f)  # noqa: E731
    out = ctypes.create_string_buffer(12 * n)
    f, g = rf(), rf()
    c = T.f12_mul(T.f12_conj(f), T.f12_inv(f))
    c = T.f12_mul(T.f12_frob(c, 2), c)  # cyclotomic subgroup element
    cases = [(0, f, T.f12_mul(f, g)), (1, f, T.f12_sqr(f)), (10, f, T.f12_mul(f, g)), (11, f, T.f12_sqr(f)), (2, f, T.f12_inv(f)),
             (3, f, T.f12_frob(f, 1)), (4, f, T.f12_frob(f, 2)), (5, f, T.f12_frob(f, 3)), (7, f, T.f12_conj(f)),
             (8, c, T.f12_pow(c, abs(cp.x))), (9, f, R.final_exp(cp, f))]
    for op, a, exp in cases:
        assert L.hm_q28c_fp12_op(cid, op, gb(a), gb(g), out) == 1, op
        assert R.gt_from_mont_bytes(cp, out.raw) == exp, op
    for reps in (() if name == "BN254" else (1, 2, 17, 63)):  # compressed squarings: the BLS12 chains only
        assert L.hm_q28c_fp12_op(cid, 12, gb(c), bytes([reps]) + bytes(12 * n - 1), out) == 1
        exp = c
        for _ in range(reps):
            exp = T.f12_sqr(exp)
        assert R.gt_from_mont_bytes(cp, out.raw) == exp, reps
    # the sparse D-twist line c0 + c3 w + c4 v w against the full product
    l0, l3, l4 = [(d.below(cp.p), d.below(cp.p)) for _ in range(3)]
    zero = (0, 0)
    line = (l0, l3, zero, l4, zero, zero)  # pyref keeps an Fp12 in the w-basis: c0 + c3 w + c4 (v w = w^3)
    lb = b"".join(R.fp_to_mont_bytes(cp, x[0]) + R.fp_to_mont_bytes(cp, x[1]) for x in (l0, l3, l4))
    assert L.hm_q28c_fp12_op(cid, 13, gb(f), lb, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == T.f12_mul(f, line)
    one = tuple([(1, 0)] + [(0, 0)] * 5)
    assert L.hm_q28c_fp12_op(cid, 9, gb(one), None, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one
    # whole pairings
    P, Q = R.random_g1(cp, d), R.random_g2(cp, d)
    P2, Q2 = R.random_g1(cp, d), R.random_g2(cp, d)
    g1, g2 = R.g1_to_mont_bytes(cp, P), R.g2_to_mont_bytes(cp, Q)
    assert L.hm_q28c_pairing(cid, g1, g2, 1, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)
    assert L.hm_q28c_pairing(cid, g1, g2, 1, 0, out) == 1
    assert R.final_exp(cp, R.gt_from_mont_bytes(cp, out.raw)) == R.pairing(cp, P, Q)
    assert L.hm_q28c_pairing(cid, g1 + R.g1_to_mont_bytes(cp, P2), g2 + R.g2_to_mont_bytes(cp, Q2), 2, 1, out) == 1
    assert R.gt_from_mont_bytes(cp, out.raw) == R.final_exp(cp, R.miller_loop(cp, [(P, Q), (P2, Q2)]))
    assert L.hm_q28c_pairing(cid, g1 + bytes(2 * n), g2 + R.g2_to_mont_bytes(cp, Q2), 2, 1, out) == 1  # second pair not live
    assert R.gt_from_mont_bytes(cp, out.raw) == R.pairing(cp, P, Q)
    gold = load_golden(name)
    c0 = gold["pairing"][0]
    assert L.hm_q28c_pairing(cid, bytes.fromhex(c0["g1"]), bytes.fromhex(c0["g2"]), 1, 1, out) == 1
    assert out.raw.hex() == c0["fexp"]
    assert L.hm_q28c_pairing(cid, bytes(2 * n), g2, 1, 1, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one
    assert L.hm_q28c_pairing(cid, g1, bytes(4 * n), 1, 1, out) == 1 and R.gt_from_mont_bytes(cp, out.raw) == one
