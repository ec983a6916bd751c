"""Operands of the device field-arithmetic tests (tests/test_devmath_host.py, tests/test_devmath_gpu.py), the Python
statement of what every op must return, and the check that every operand respects the op's contract.

Per op and curve: a structured block of a few thousand vectors (the limb patterns and weight boundaries that set particular
carries and bring column sums just under 2^63) followed by uniform random vectors up to N_VECTORS.  Deterministic: every
random draw comes from a numpy generator seeded by oracle.pyref.Drbg.

The contract (csrc/fp28.h, "Invariants") as used here:
  * normalized: limbs 0..L-2 in [0, 2^28), value in (-0.2 p, 1.2 p);
  * weight w: a sum / difference of w normalized values, so |limb_i| < w 2^28 for i < L-1 and |value| < 1.2 w p -- the TOP
    limb is bounded through the value, not by w 2^28 (a top limb of 2^28 would be a value of R28 / 2^28, thousands of p);
  * fp28_mul: w_a w_b <= 8; fp28_mul2: w_a w_b + w_c w_d <= 8; fp28_sqr: w_a <= 2; fp28_k2mul: all four normalized;
  * every column of the product scanning stays below 2^63 in magnitude.  check_preconditions verifies the stronger
    statement that the SUM OF THE MAGNITUDES of a column's terms (incoming carry, limb products, m p terms) is below 2^63,
    which bounds every partial sum in whatever order a multiplier adds them -- exactly, in 64-bit unsigned integers for
    all vectors, and with Python integers along fp28_mont's own order of additions for the structured block.
"""
import functools
import os
import subprocess

import numpy as np

from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
N_VECTORS = 1 << 16
B28 = 1 << 28
M28 = B28 - 1
LIM63 = 1 << 63

# op codes of tests/devmath/devmath.hip (dm_run) and, from 16 on, of tests/hostmath/hostmath.cpp (hm_fp28_raw)
OPS = {
    "fp_mul": 0, "fp_mul_i": 1, "fp_sqr": 2, "fp_mul2": 3, "fp_mul_inline": 4, "fp_add": 5, "fp_sub": 6, "fp_neg": 7, "fp_inv": 8,
    "fp28_mul": 16, "fp28_sqr": 17, "fp28_mul2": 18, "fp28_k2mul": 19, "fp28_normalize": 20, "fp28_reduce": 21,
    "fp28_from_fp": 22, "fp28_to_fp": 23,
}
SAT_ARITY = {"fp_mul": 2, "fp_mul_i": 2, "fp_sqr": 1, "fp_mul2": 4, "fp_mul_inline": 2, "fp_add": 2, "fp_sub": 2, "fp_neg": 1, "fp_inv": 1}


class Field:
    """the constants of one curve's two representations, derived from p alone (independent of curve_constants.h)"""

    def __init__(self, name):
        cp = R.CURVES[name]
        self.name, self.cp, self.cid, self.p = name, cp, cp.curve_id, cp.p
        self.N = cp.fp_bytes // 4
        self.L = {8: 10, 12: 14}[self.N]
        self.R = 1 << (32 * self.N)
        self.R28 = 1 << (28 * self.L)
        self.s = 28 * (self.L - 1)  # the top limb's shift
        self.P28 = [(self.p >> (28 * i)) & M28 for i in range(self.L - 1)] + [self.p >> self.s]
        self.PINV28 = (-pow(self.p, -1, B28)) % B28
        # value in (-0.2 p, 1.2 p)  <=>  norm_lo <= value < norm_hi  (p is not a multiple of 5)
        self.norm_lo, self.norm_hi = -(self.p // 5), 6 * self.p // 5 + 1

    def weight_bound(self, w):
        """|value| < 1.2 w p  <=>  |value| <= this"""
        return 6 * w * self.p // 5


@functools.lru_cache(maxsize=None)
def field(name):
    return Field(name)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness(portable: bool) -> str:
    """hipcc build of tests/devmath/devmath.hip with the product's own flags (mathlib_amd.build.FLAGS), as shipped or with
    -DMLHIP_FP28_PORTABLE; cached by mtime against the source and the csrc headers.  Returns the library's path."""
    from mathlib_amd import build as B

    d = os.path.join(ROOT, "tests", "devmath")
    src = os.path.join(d, "devmath.hip")
    so = os.path.join(d, "libdevmath_portable.so" if portable else "libdevmath.so")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(B.CSRC, f)) for f in os.listdir(B.CSRC) if f.endswith((".h", ".inc"))])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        cmd = [B._hipcc()] + B.FLAGS + ["-shared", "-I", B.CSRC] + (["-DMLHIP_FP28_PORTABLE"] if portable else []) + ["-o", so, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, "hipcc failed for the device harness:\n%s\n%s" % (r.stdout, r.stderr)
    return so


def _rng(stream):
    return np.random.Generator(np.random.PCG64(int.from_bytes(R.Drbg("devmath/" + stream).block(), "big")))


# ---- conversions -------------------------------------------------------------------------------------------------------
def sat_array(vals, N):
    """integers in [0, 2^(32 N)) -> uint32[n, N], little-endian limbs"""
    return np.frombuffer(b"".join(v.to_bytes(4 * N, "little") for v in vals), dtype="<u4").reshape(-1, N).copy()


def sat_ints(arr):
    N = arr.shape[1]
    raw = np.ascontiguousarray(arr, dtype="<u4").tobytes()
    return [int.from_bytes(raw[i : i + 4 * N], "little") for i in range(0, len(raw), 4 * N)]


def limbs_of(v, L):
    """the normalized limbs of an integer: limbs 0..L-2 in [0, 2^28), the signed rest on top"""
    return [(v >> (28 * i)) & M28 for i in range(L - 1)] + [v >> (28 * (L - 1))]


def limb_array(rows):
    a = np.array(rows, dtype=np.int64)
    assert a.size == 0 or (np.abs(a) < (1 << 31)).all()
    return a.astype(np.int32)


def values(arr):
    """int32[n, L] raw limbs -> object array of the Python integers sum_i l_i 2^(28 i)"""
    a = arr.astype(np.int64).astype(object)
    v = a[:, -1]
    for i in range(arr.shape[1] - 2, -1, -1):
        v = (v << 28) + a[:, i]
    return v


def normalize_np(arr):
    """fp28_normalize on int64: the unique representation with limbs 0..L-2 in [0, 2^28)"""
    a = arr.astype(np.int64)
    out = np.empty_like(a)
    c = np.zeros(len(a), dtype=np.int64)
    for i in range(a.shape[1] - 1):
        v = a[:, i] + c
        out[:, i] = v & M28
        c = v >> 28
    out[:, -1] = a[:, -1] + c
    return out


def in_range(arr, lo, hi):
    """lo <= value < hi for every row, exactly: lexicographic comparison of the normalized limbs from the top"""
    L = arr.shape[1]
    nrm = normalize_np(arr)

    def less(bound):
        b = limbs_of(bound, L)
        lt = np.zeros(len(nrm), dtype=bool)
        eq = np.ones(len(nrm), dtype=bool)
        for i in range(L - 1, -1, -1):
            lt |= eq & (nrm[:, i] < b[i])
            eq &= nrm[:, i] == b[i]
        return lt

    return ~less(lo) & less(hi)


def low_limbs_normalized(arr):
    low = arr[:, :-1]
    return ((low >= 0) & (low < B28)).all(axis=1)


def is_normalized(F, arr):
    """the predicate of fp28.h:14-15 for every row"""
    return low_limbs_normalized(arr) & in_range(arr, F.norm_lo, F.norm_hi)


def has_weight(F, arr, w):
    b = F.weight_bound(w)
    return (np.abs(arr[:, :-1].astype(np.int64)) < w * B28).all(axis=1) & in_range(arr, -b, b + 1)


# ---- the algorithm as written in fp28.h, in Python integers ------------------------------------------------------------
def _i32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


class _Acc:
    """a 64-bit accumulator that refuses to overflow and remembers its largest magnitude"""

    def __init__(self):
        self.v, self.worst = 0, 0

    def add(self, x):
        self.v += x
        self.worst = max(self.worst, abs(self.v))
        if not -LIM63 <= self.v < LIM63:
            raise OverflowError("a column sum left the 64-bit accumulator")


def mont_py(F, a, b=None, c=None, d=None, sqr=False):
    """fp28_mont<C, DUAL, SQR>, addition by addition: (limbs, largest |accumulator|).  DUAL when c is given."""
    L, P = F.L, F.P28
    acc = _Acc()
    m, t = [0] * L, [0] * L
    a2 = [_i32(x + x) for x in a] if sqr else None
    for k in range(2 * L - 1):
        lo, hi = (0, k) if k < L else (k - L + 1, L - 1)
        if sqr:
            for i in range(lo, hi + 1):
                j = k - i
                if i < j:
                    acc.add(a[i] * a2[j])
                if i == j:
                    acc.add(a[i] * a[i])
        else:
            for i in range(lo, hi + 1):
                acc.add(a[i] * b[k - i])
            if c is not None:
                for i in range(lo, hi + 1):
                    acc.add(c[i] * d[k - i])
        for i in range(lo, hi + 1):
            if k < L and i == k:
                continue
            acc.add(m[i] * P[k - i])
        if k < L:
            m[k] = (((acc.v & 0xFFFFFFFF) * F.PINV28) & 0xFFFFFFFF) & M28
            acc.add(m[k] * P[0])
        else:
            t[k - L] = acc.v & M28
        acc.v >>= 28
    t[L - 1] = _i32(acc.v)
    return t, acc.worst


def k2mul_py(F, a0, a1, b0, b1):
    """fp28_k2mul_portable, addition by addition: (c0 limbs, c1 limbs, largest |accumulator|)"""
    L, P = F.L, F.P28
    s = [_i32(x + y) for x, y in zip(a0, a1)]
    t = [_i32(x + y) for x, y in zip(b0, b1)]
    c0, c1 = _Acc(), _Acc()
    m0, m1, t0, t1 = [0] * L, [0] * L, [0] * L, [0] * L
    for k in range(2 * L - 1):
        lo, hi = (0, k) if k < L else (k - L + 1, L - 1)
        p0, p1 = _Acc(), _Acc()
        for i in range(lo, hi + 1):
            p0.add(a0[i] * b0[k - i])
            p1.add(a1[i] * b1[k - i])
            c1.add(s[i] * t[k - i])
        for i in range(lo, hi + 1):
            if k < L and i == k:
                continue
            c0.add(m0[i] * P[k - i])
            c1.add(m1[i] * P[k - i])
        d0, d1 = _Acc(), _Acc()
        d0.add(p0.v - p1.v)
        d1.add(p0.v + p1.v)
        c0.add(d0.v)
        c1.add(-d1.v)
        if k < L:
            m0[k] = (((c0.v & 0xFFFFFFFF) * F.PINV28) & 0xFFFFFFFF) & M28
            c0.add(m0[k] * P[0])
            m1[k] = (((c1.v & 0xFFFFFFFF) * F.PINV28) & 0xFFFFFFFF) & M28
            c1.add(m1[k] * P[0])
        else:
            t0[k - L] = c0.v & M28
            t1[k - L] = c1.v & M28
        c0.v >>= 28
        c1.v >>= 28
    t0[L - 1], t1[L - 1] = _i32(c0.v), _i32(c1.v)
    return t0, t1, max(x.worst for x in (c0, c1))


def transcription(F, op, v):
    """the output limb lists of a product op on one vector of limb lists, by the transcriptions above"""
    if op == "fp28_k2mul":
        return list(k2mul_py(F, *v)[:2])
    if op == "fp28_sqr":
        return [mont_py(F, v[0], sqr=True)[0]]
    return [mont_py(F, *v)[0]]


def product_integers(op, vals):
    """per output, the integers W with  output R28 = W (mod p);  vals: the operands' values (integers or object arrays)"""
    if op == "fp28_mul":
        return [vals[0] * vals[1]]
    if op == "fp28_sqr":
        return [vals[0] * vals[0]]
    if op == "fp28_mul2":
        return [vals[0] * vals[1] + vals[2] * vals[3]]
    if op == "fp28_k2mul":  # (a0 + a1 u)(b0 + b1 u), u^2 = -1
        a0, a1, b0, b1 = vals
        return [a0 * b0 - a1 * b1, a0 * b1 + a1 * b0]
    raise KeyError(op)


# ---- the same columns for all vectors at once: magnitudes in exact 64-bit unsigned arithmetic ----------------------------
def _mag(x):
    return np.abs(x.astype(np.int64)).astype(np.uint64)


def column_magnitudes(F, op, ops):
    """For every vector the largest, over the columns, SUM OF MAGNITUDES of the terms the column adds up (|incoming carry| +
    sum |limb products| + sum m_i p_j), as uint64.  Exact as long as the declared weights hold (the sums then stay below
    2^64; check_preconditions tests the weights first); the m_i and carries come from the exact signed run alongside,
    which cannot overflow when the magnitudes stay below 2^63."""
    L, P = F.L, [np.int64(x) for x in F.P28]
    n = len(ops[0])
    if op == "fp28_k2mul":
        a0, a1, b0, b1 = (x.astype(np.int64) for x in ops)
        chains = [[(a0, b0, 1), (a1, b1, -1)], [(a0 + a1, b0 + b1, 1), (a0, b0, -1), (a1, b1, -1)]]
    elif op == "fp28_sqr":
        a = ops[0].astype(np.int64)
        chains = [[(a, a, 1)]]
    else:
        x = [o.astype(np.int64) for o in ops]
        chains = [[(x[i], x[i + 1], 1) for i in range(0, len(x), 2)]]
    worst = np.zeros(n, dtype=np.uint64)
    for prods in chains:
        acc = np.zeros(n, dtype=np.int64)
        m = np.zeros((n, L), dtype=np.int64)
        for k in range(2 * L - 1):
            lo, hi = (0, k) if k < L else (k - L + 1, L - 1)
            mag = _mag(acc)
            for u, v, sgn in prods:
                for i in range(lo, hi + 1):
                    acc += sgn * u[:, i] * v[:, k - i]
                    mag += _mag(u[:, i]) * _mag(v[:, k - i])
            for i in range(lo, hi + 1):
                if k < L and i == k:
                    continue
                acc += m[:, i] * P[k - i]
                mag += (m[:, i] * P[k - i]).astype(np.uint64)
            if k < L:
                m[:, k] = ((acc & M28) * np.int64(F.PINV28)) & M28
                acc += m[:, k] * P[0]
                mag += (m[:, k] * P[0]).astype(np.uint64)
            worst = np.maximum(worst, mag)
            acc >>= 28
    return worst


# ---- structured values ---------------------------------------------------------------------------------------------------
def sat_structured(F):
    """(all structured values, the short list whose pairs are all formed), canonical integers < p"""
    p, N = F.p, F.N
    bits = p.bit_length()
    short = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, F.R % p, F.R * F.R % p]
    pw = []
    for k32 in range(0, 32 * N + 1, 32):
        for k in (k32 - 1, k32, k32 + 1):
            if 0 <= k and (1 << k) < p:
                pw += [1 << k, p - (1 << k)]
    pats = []
    for mask in range(1 << N):  # limbs each 0 or 0xFFFFFFFF
        v = sum(0xFFFFFFFF << (32 * i) for i in range(N) if (mask >> i) & 1)
        if v < p:
            pats.append(v)
    one = []
    for i in range(N):  # one nonzero limb
        for x in (1, 0x80000000, 0xFFFFFFFF, 0x55555555):
            if (x << (32 * i)) < p:
                one.append(x << (32 * i))
    top = p >> (32 * (N - 1))
    one += [top << (32 * (N - 1)), (top - 1) << (32 * (N - 1))]
    assert bits > 32 * (N - 1)
    short += [1 << (32 * i) for i in range(1, N)] + [p - (1 << (32 * i)) for i in range(1, N)]
    short += [0xFFFFFFFF << (32 * i) for i in range(N - 1)] + [(1 << (32 * (N - 1))) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1]
    allv = list(dict.fromkeys(short + pw + pats + one))
    short = list(dict.fromkeys(short))
    assert all(0 <= v < p for v in allv)
    return allv, short


def _fit_top(F, low, w, sign):
    """the extreme top limb (largest for sign > 0, smallest for sign < 0) that keeps low + top 2^s inside +-1.2 w p"""
    b = F.weight_bound(w)
    lowsum = sum(x << (28 * i) for i, x in enumerate(low))
    return (b - lowsum) >> F.s if sign > 0 else -((b + lowsum) >> F.s)


def weighted_patterns(F, w):
    """weight-w limb patterns: every limb at +-(w 2^28 - 1), alternating signs, one extreme limb at each position, the top
    limb alone at its extreme (the top limb's extreme is the one the value bound allows, see the module docstring)"""
    L = F.L
    e = w * B28 - 1
    rows = []
    for low, signs in (([e] * (L - 1), (1,)), ([-e] * (L - 1), (-1,)), ([e if i % 2 == 0 else -e for i in range(L - 1)], (1, -1)),
                       ([-e if i % 2 == 0 else e for i in range(L - 1)], (1, -1)), ([0] * (L - 1), (1, -1))):
        for sg in signs:
            rows.append(low + [_fit_top(F, low, w, sg)])
    for i in range(L - 1):
        for x in (e, -e):
            low = [0] * (L - 1)
            low[i] = x
            rows.append(low + [0 if i % 2 else _fit_top(F, low, w, 1 if x < 0 else -1)])
    return rows


def normalized_values(F):
    """normalized values (limbs 0..L-2 in [0, 2^28)): both ends of (-0.2 p, 1.2 p) and the usual suspects in between"""
    p, L = F.p, F.L
    v = [F.norm_lo, F.norm_lo + 1, F.norm_lo + 2, F.norm_hi - 1, F.norm_hi - 2, F.norm_hi - 3, 0, 1, -1, 2, p - 1, p, p + 1, (p - 1) // 2,
         F.R28 % p, F.R28 * F.R28 % p, F.R % p]
    v += [1 << (28 * k) for k in range(1, L - 1)] + [(1 << (28 * k)) - 1 for k in range(1, L)]
    v += [p - (1 << (28 * k)) for k in range(1, L - 1)]
    low = [M28] * (L - 1)
    v += [sum(x << (28 * i) for i, x in enumerate(low)) + (_fit_top(F, low, 1, 1) << F.s)]
    v = [x for x in dict.fromkeys(v) if F.norm_lo <= x < F.norm_hi]
    return [limbs_of(x, L) for x in v]


# ---- random values -------------------------------------------------------------------------------------------------------
def sat_random(F, rng, n):
    """uniform limbs with the top limb below p's: uniform over the values < p whose top limb is not p's own"""
    a = rng.integers(0, 1 << 32, size=(n, F.N), dtype=np.uint64)
    a[:, -1] = rng.integers(0, F.p >> (32 * (F.N - 1)), size=n, dtype=np.uint64)
    return a.astype(np.uint32)


def normalized_random(F, rng, n):
    """y uniform below p (as above), moved by +-p where that stays inside (-0.2 p, 1.2 p): all of the normalized range"""
    y = rng.integers(0, B28, size=(n, F.L), dtype=np.int64)
    y[:, -1] = rng.integers(0, F.P28[-1], size=n, dtype=np.int64)
    pl = np.array(F.P28, dtype=np.int64)
    which = rng.integers(0, 3, size=n)
    out = y.copy()
    for sel, cand in ((1, normalize_np(y - pl)), (2, normalize_np(y + pl))):
        ok = (which == sel) & in_range(cand, F.norm_lo, F.norm_hi)
        out[ok] = cand[ok]
    return out.astype(np.int32)


def weighted_random(F, rng, n, w):
    """a signed sum of w normalized values, limb by limb without carry propagation"""
    acc = np.zeros((n, F.L), dtype=np.int64)
    for _ in range(w):
        sg = rng.integers(0, 2, size=(n, 1)) * 2 - 1
        acc += sg * normalized_random(F, rng, n)
    return acc.astype(np.int32)


# ---- the operand sets ------------------------------------------------------------------------------------------------------
MUL_WEIGHTS = [(1, 8), (2, 4), (4, 2), (8, 1)]
SQR_WEIGHTS = [1, 2]


def mul2_weights():
    """every (w_a, w_b, w_c, w_d) with w_a w_b + w_c w_d = 8"""
    out = []
    for s in range(1, 8):
        for wa in range(1, s + 1):
            if s % wa == 0:
                for wc in range(1, 8 - s + 1):
                    if (8 - s) % wc == 0:
                        out.append((wa, s // wa, wc, (8 - s) // wc))
    return out


def _freeze(arrs):
    for a in arrs:
        a.setflags(write=False)
    return tuple(arrs)


class Cases:
    """operands: tuple of arrays [n, N or L]; weights: int array [n, arity] (fp28 ops; 0 = 'normalized' for k2mul);
    n_struct: length of the structured block in front; sample: indices of a few hundred structured vectors"""

    def __init__(self, op, operands, weights, n_struct):
        self.op, self.operands, self.weights, self.n_struct = op, _freeze(list(operands)), weights, n_struct
        self.n = len(operands[0])
        step = max(1, n_struct // 300)
        self.sample = np.arange(0, n_struct, step)


def _sat_cases(F, op):
    ar = SAT_ARITY[op]
    allv, short = sat_structured(F)
    if op == "fp_inv":
        # the structured list plus values whose gcd chains are long (consecutive Fibonacci numbers)
        a, b = 1, 2
        while b < F.p:
            a, b = b, a + b
        cols = [allv + [a, b - a, F.p - a, pow(F.R, -1, F.p)]]
    elif ar == 1:
        cols = [allv]
    else:
        pairs = [(x, y) for x in short for y in short]
        pairs += [(x, allv[(7 * i + 3) % len(allv)]) for i, x in enumerate(allv)] + [(x, x) for x in allv]
        cols = [[x for x, _ in pairs], [y for _, y in pairs]]
        if ar == 4:
            k = len(pairs) // 3
            rot = pairs[k:] + pairs[:k]
            cols += [[x for x, _ in rot], [y for _, y in rot]]
    ns = len(cols[0])
    # the inversion is ~30 k instructions a lane and its reference a pow() each: a smaller random block
    total = 4096 if op == "fp_inv" else N_VECTORS
    rng = _rng("%s/%s" % (F.name, op))
    arrs = [np.concatenate([sat_array(c, F.N), sat_random(F, rng, total - ns)]) for c in cols]
    return Cases(op, arrs, None, ns)


def _fp28_cases(F, op):
    rng = _rng("%s/%s" % (F.name, op))
    L = F.L
    nrm = normalized_values(F)
    rows, wts = [], []  # rows: tuples of limb lists

    def add(vec, w):
        rows.append(vec)
        wts.append(w)

    if op == "fp28_mul":
        for wa, wb in MUL_WEIGHTS:
            for x in weighted_patterns(F, wa):
                for y in weighted_patterns(F, wb):
                    add((x, y), (wa, wb))
        for x in nrm:
            for y in nrm:
                add((x, y), (1, 1))
        rand_w = MUL_WEIGHTS + [(1, 1), (2, 2)]
    elif op == "fp28_sqr":
        for w in SQR_WEIGHTS:
            for x in weighted_patterns(F, w):
                add((x,), (w,))
        for x in nrm:
            add((x,), (1,))
        rand_w = [(1,), (2,)]
    elif op == "fp28_mul2":
        for ws in mul2_weights():
            pats = [weighted_patterns(F, w) for w in ws]
            # all four at their extremes in every sign combination (the column sums just under 2^63 in both directions and
            # the complete cancellations), then the patterns walked in step
            for sg in range(16):
                add(tuple(pats[j][1 if (sg >> j) & 1 else 0] for j in range(4)), ws)
            for i in range(len(pats[0])):
                add(tuple(pats[j][(i + 3 * j) % len(pats[j])] for j in range(4)), ws)
        for i, x in enumerate(nrm):
            add((x, nrm[(i + 1) % len(nrm)], nrm[(i + 2) % len(nrm)], nrm[(i + 3) % len(nrm)]), (1, 1, 1, 1))
        rand_w = mul2_weights() + [(1, 1, 1, 1)]
    elif op == "fp28_k2mul":
        def comp(x):  # p - x: normalized again, and x + comp(x) = p
            return limbs_of(F.p - sum(v << (28 * i) for i, v in enumerate(x)), L)

        for x in nrm:
            for y in nrm:
                for vec in ((x, y, y, x), (x, comp(x), y, y), (x, x, y, y), (x, comp(x), y, comp(y))):
                    add(vec, (1, 1, 1, 1))
        rand_w = [(1, 1, 1, 1)]
    elif op == "fp28_to_fp":
        for w in (1, 2, 4, 8):
            for x in weighted_patterns(F, w):
                add((x,), (w,))
        for x in nrm:
            add((x,), (1,))
        rand_w = [(1,), (2,), (4,), (8,), (8,)]
    elif op == "fp28_normalize":
        # 32-bit carries: limb + carry must stay inside int32, which every sum of 8 normalized values does (limbs in
        # [-8 (2^28 - 1), 8 (2^28 - 1)], carries in [-8, 7]) but -(8 2^28 - 1) with a carry of -8 does not: the patterns at
        # +-(w 2^28 - 1) stop at weight 7, weight 8 comes as the attainable extreme +-8 (2^28 - 1)
        for w in (1, 2, 4, 7):
            for x in weighted_patterns(F, w):
                add((x,), (w,))
        e = 8 * (B28 - 1)
        for low in ([e] * (L - 1), [-e] * (L - 1), [e if i % 2 else -e for i in range(L - 1)]):
            add((low + [0],), (8,))
        rand_w = [(2,), (4,), (8,)]
    else:
        raise KeyError(op)
    ar = len(rows[0])
    ns = len(rows)
    fill = N_VECTORS - ns
    assert fill > 0
    per = -(-fill // len(rand_w))
    rnd = [[] for _ in range(ar)]
    rw = []
    for ws in rand_w:
        for j, w in enumerate(ws):
            rnd[j].append(normalized_random(F, rng, per) if w == 1 and op == "fp28_k2mul" else weighted_random(F, rng, per, w))
        rw += [ws] * per
    arrs = [np.concatenate([limb_array([r[j] for r in rows])] + rnd[j])[:N_VECTORS] for j in range(ar)]
    weights = np.array(wts + rw, dtype=np.int64)[:N_VECTORS]
    return Cases(op, arrs, weights, ns)


def _reduce_cases(F):
    """the inputs of tests/test_host_math.py::test_fp28_reduce_range for any curve: values up to +-600 p, every third one
    with un-normalized limbs of weight up to 8; then the same shapes drawn at random"""
    L, p = F.L, F.p
    d = R.Drbg("devmath/reduce/" + F.name)
    rows = []
    for trial in range(1200):
        scale = [1, 2, 7, 50, 300, 600][trial % 6]
        v = d.below(2 * scale * p) - scale * p
        limbs, rest = [], v
        for _ in range(L - 1):
            l = rest & M28
            if trial % 3 == 1:
                l += (d.below(15) - 7) << 28
            limbs.append(l)
            rest = (rest - l) >> 28
        limbs.append(rest)
        assert sum(l << (28 * i) for i, l in enumerate(limbs)) == v
        rows.append(limbs)
    for scale in (1, 600):  # the ends themselves
        for v in (scale * p, -scale * p, scale * p - 1, -scale * p + 1, scale * p - p // 2, scale * p - p // 2 - 1):
            rows.append(limbs_of(v, L))
    ns = len(rows)
    rng = _rng("%s/reduce" % F.name)
    n = N_VECTORS - ns
    a = rng.integers(0, B28, size=(n, L), dtype=np.int64)
    ptop = F.p / (1 << F.s)  # p in units of the top limb
    scale = np.array([1, 2, 7, 50, 300, 599])[rng.integers(0, 6, size=n)]
    a[:, -1] = np.floor((rng.random(n) * 2 - 1) * scale * ptop).astype(np.int64)
    extra = rng.integers(-7, 7, size=(n, L - 1)) << 28
    extra[rng.integers(0, 3, size=n) != 1] = 0
    # the value is kept: what the lower limbs gain, the next limb gives back
    a[:, :-1] += extra
    a[:, 1:] -= extra >> 28
    arr = np.concatenate([limb_array(rows), a.astype(np.int32)])
    return Cases("fp28_reduce", [arr], None, ns)


def _from_fp_cases(F):
    allv, _ = sat_structured(F)
    rng = _rng("%s/from_fp" % F.name)
    arr = np.concatenate([sat_array(allv, F.N), sat_random(F, rng, N_VECTORS - len(allv))])
    return Cases("fp28_from_fp", [arr], None, len(allv))


@functools.lru_cache(maxsize=None)
def cases(name, op):
    F = field(name)
    if op in SAT_ARITY:
        return _sat_cases(F, op)
    if op == "fp28_reduce":
        return _reduce_cases(F)
    if op == "fp28_from_fp":
        return _from_fp_cases(F)
    return _fp28_cases(F, op)


ALL_OPS = list(OPS)


# ---- the contract ------------------------------------------------------------------------------------------------------
def _below_p(F, arr):
    nrm = arr.astype(np.int64)
    b = [(F.p >> (32 * i)) & 0xFFFFFFFF for i in range(F.N)]
    lt = np.zeros(len(nrm), dtype=bool)
    eq = np.ones(len(nrm), dtype=bool)
    for i in range(F.N - 1, -1, -1):
        lt |= eq & (nrm[:, i] < b[i])
        eq &= nrm[:, i] == b[i]
    return lt


def check_preconditions(name, op):
    """Raises ValueError when a vector of cases(name, op) is outside what the op accepts; returns the largest column
    magnitude found (0 for ops without columns) so that a test can see how close to 2^63 the block gets."""
    F = field(name)
    cs = cases(name, op)
    if not all(len(a) == cs.n for a in cs.operands):
        raise ValueError("%s %s: operand arrays of different lengths" % (name, op))

    def bad(what, mask):
        if not mask.all():
            raise ValueError("%s %s: vector %d: %s" % (name, op, int(np.flatnonzero(~mask)[0]), what))

    if op in SAT_ARITY or op == "fp28_from_fp":
        for a in cs.operands:
            bad("operand not below p", _below_p(F, a))
        return 0
    if op == "fp28_reduce":
        a = cs.operands[0]
        bad("limb above weight 8", (np.abs(a[:, :-1].astype(np.int64)) < 8 * B28).all(axis=1))
        bad("|value| above 601 p", in_range(a, -601 * F.p, 601 * F.p))
        return 0
    W = cs.weights
    for j, a in enumerate(cs.operands):
        for w in np.unique(W[:, j]):
            sel = W[:, j] == w
            ok = np.ones(cs.n, dtype=bool)
            ok[sel] = has_weight(F, a[sel], int(w))
            bad("operand %d is not of weight %d" % (j, w), ok)
    if op == "fp28_mul":
        bad("w_a w_b > 8", W[:, 0] * W[:, 1] <= 8)
    elif op == "fp28_mul2":
        bad("w_a w_b + w_c w_d > 8", W[:, 0] * W[:, 1] + W[:, 2] * W[:, 3] <= 8)
    elif op == "fp28_sqr":
        bad("w_a > 2", W[:, 0] <= 2)
    elif op == "fp28_k2mul":
        for j, a in enumerate(cs.operands):
            bad("operand %d is not normalized" % j, is_normalized(F, a))
    elif op == "fp28_to_fp":
        bad("w_a > 8", W[:, 0] <= 8)
    if op in ("fp28_normalize",):
        return 0
    ops = cs.operands
    if op == "fp28_to_fp":  # fp28_mul(a, FROM28): FROM28 = R mod p, canonical
        k = limb_array([limbs_of(F.R % F.p, F.L)])
        ops = (ops[0], np.repeat(k, cs.n, axis=0))
        colop = "fp28_mul"
    else:
        colop = op
    mags = column_magnitudes(F, colop, ops)
    bad("a column's magnitudes sum to 2^63 or more", mags < np.uint64(LIM63))
    # the structured sample again in Python integers, along the order of additions of fp28.h
    for i in cs.sample:
        v = [[int(x) for x in o[i]] for o in ops]
        try:
            if colop == "fp28_k2mul":
                w_ = k2mul_py(F, *v)[2]
            elif colop == "fp28_sqr":
                w_ = mont_py(F, v[0], sqr=True)[1]
            else:
                w_ = mont_py(F, *v)[1]
        except OverflowError as e:
            raise ValueError("%s %s: vector %d: %s" % (name, op, int(i), e))
        if w_ > int(mags[i]):
            raise ValueError("%s %s: vector %d: a partial sum exceeds the sum of magnitudes" % (name, op, int(i)))
    return int(mags.max())
