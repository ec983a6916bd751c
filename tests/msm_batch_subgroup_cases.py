"""Inputs of the tests of mlhip_msm_batch* with MLHIP_CURVE_SUBGROUP_POINTS (tests/test_msm_batch_subgroup_host.py,
tests/test_msm_batch_subgroup_gpu.py): which (curve, group) has a split, the scalars that sit on the digit boundaries of the
split, the degenerate pairs the split chunks add to those of tests/msm_batch_cases.py, and the host build of the chunk
bodies (tests/hostmath_batch_endo).  Expected bytes are msm_batch_cases.expected's (cref.msm of every segment)."""
import ctypes
import functools
import os
import random
import subprocess

from conftest import ROOT
from gt_exp_cyclo_cases import boundary_scalars, split_modulus
from msm_batch_cases import neg_point, point_bytes, sc
from oracle import pyref as R
from point_sum_cases import distinct_points

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
# (BN254 G1: E(Fp) has prime order and no short split without a lattice reduction -- the flag is accepted and ignored)
SPLIT = [("BN254", 2), ("BLS12-381", 1), ("BLS12-381", 2), ("BLS12-377", 1), ("BLS12-377", 2)]
# the chunk lengths the split chunks are compiled for
CHUNKS = {1: (1, 2, 4, 8), 2: (1, 2, 4)}


def endo_scalar(cp, group):
    """lambda with [lambda]P = the endomorphism image the chunk adds for the digit after the first: x^2 on G1 of a BLS12
    curve ((beta x, -y)), |x| / 6 x^2 on G2 (+-psi Q)"""
    return cp.x * cp.x if group == 1 else split_modulus(cp)[0]


def harness():
    """the ctypes handle of tests/hostmath_batch_endo, built when it is older than the headers"""
    d = os.path.join(ROOT, "tests", "hostmath_batch_endo")
    so = os.path.join(d, "libhostmath_batch_endo.so")
    src = os.path.join(d, "batch_endo.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hbe_msm_batch.argtypes = [ci, ci, ci, vp, vp, ci, vp, ctypes.c_size_t, vp]
    return lib


def offsets_of(lengths):
    offs = (ctypes.c_uint64 * (len(lengths) + 1))()
    for i, m in enumerate(lengths):
        offs[i + 1] = offs[i] + m
    return offs


def host_batch(lib, cp, group, P, pts, scs, lengths, mont):
    """(return code, the affine sum of every segment by the split chunk bodies on the CPU)"""
    ps = point_bytes(cp, group)
    out = ctypes.create_string_buffer(max(1, len(lengths)) * ps)
    rc = lib.hbe_msm_batch(cp.curve_id, group, P, pts, scs, 1 if mont else 0, offsets_of(lengths), len(lengths), out)
    return rc, [out.raw[i * ps : (i + 1) * ps] for i in range(len(lengths))]


def to_bytes(cp, group, pt):
    return R.g1_to_mont_bytes(cp, pt) if group == 1 else R.g2_to_mont_bytes(cp, pt)


def mul(cp, group, pt, k):
    return R.g1_mul(cp, pt, k) if group == 1 else R.g2_mul(cp, pt, k)


@functools.lru_cache(maxsize=None)
def special_scalars(name, group):
    """the boundary scalars of the split; a = 0 and b = 0 of the G1 split (s = b x^2, s < x^2) and single non-zero digits of
    the G2 split; values below 2^64 and 2^128; unreduced values"""
    cp = R.CURVES[name]
    d = R.Drbg("msm_batch_subgroup/scalars/%s/%d" % (name, group))
    lam, dim = split_modulus(cp)
    one_digit = [d.below(lam) * lam**k for k in range(dim)]
    g1_halves = [d.below(1 << 120) * cp.x * cp.x, d.below(cp.x * cp.x), cp.x * cp.x, cp.x * cp.x - 1]
    reduced = boundary_scalars(cp) + [v % cp.r for v in one_digit + g1_halves] + [d.below(1 << 64), d.below(1 << 128), d.below(cp.r)]
    unreduced = [cp.r, cp.r + 1, 2 * cp.r + 3, (1 << 256) - 1]
    return tuple(reduced), tuple(unreduced)


@functools.lru_cache(maxsize=None)
def scalar_segments(name, group, mont):
    """(points, scalars, lengths): every special scalar once over distinct points of the subgroup, an infinity among them,
    in segments of lengths 1, 2, 3, 5, 8, 4, 7, ... -- every count below and at every compiled P.  Reduced values keep their
    meaning in both scalar forms (mont: their Montgomery form); the unreduced ones are taken as they are."""
    cp = R.CURVES[name]
    reduced, unreduced = special_scalars(name, group)
    raw = [R.scalar_to_bytes(s, cp, mont=bool(mont)) for s in reduced] + [s.to_bytes(32, "little") for s in unreduced]
    n = len(raw)
    pts = list(distinct_points(name, group, 300)[:n])
    pts[n // 3] = None
    lengths, left, cyc = [], n, 0
    while left:
        m = min(left, (1, 2, 3, 5, 8, 4, 7)[cyc % 7])
        lengths.append(m)
        left -= m
        cyc += 1
    return b"".join(to_bytes(cp, group, p) for p in pts), b"".join(raw), tuple(lengths)


def endo_edge_segments(cp, group, seed, pad=0):
    """degenerate pairs the split adds, side by side in one chunk (P >= 2), pad pairs of the subgroup in front of each so
    that they also straddle chunk boundaries.  With lambda = endo_scalar and Q = [lambda]P:
      (P, d lambda) beside (Q, d)      both add the same point at the same loop positions: the accumulator meets its own
                                       table entry through the endomorphism (the doubling branch)
      (P, d lambda) beside (-Q, d)     the same pair cancelling to infinity
      (P, d), (Q, d), ([lambda]Q, d)   images of one point in neighbouring pairs (G2: psi, psi^2)
      (P, e + d lambda) beside (Q, r - d)   cancels down to [e]P"""
    rnd = random.Random(seed)
    name = cp.name
    lam = endo_scalar(cp, group)
    base = distinct_points(name, group, 300)
    P0 = base[7]
    Q = mul(cp, group, P0, lam % cp.r)
    Q2 = mul(cp, group, Q, lam % cp.r)
    bP, bQ, bQ2 = (to_bytes(cp, group, p) for p in (P0, Q, Q2))
    d = rnd.randrange(1, min(lam, 1 << 100))
    e = rnd.randrange(1, lam)
    assert d * lam + e < cp.r
    cases = [
        ([bP, bQ], [d * lam, d]),
        ([bQ, bP], [d, d * lam]),
        ([bP, neg_point(cp, group, bQ)], [d * lam, d]),
        ([bP, bQ, bQ2], [d, d, d]),
        ([bP, bQ, bP, bQ], [d * lam, d, d * lam, d]),
        ([bP, bQ], [e + d * lam, cp.r - d]),
        ([bP, bQ], [1, 1]),
        ([bQ, neg_point(cp, group, bQ)], [lam, lam]),
    ]
    pad_pts = [to_bytes(cp, group, base[9]), to_bytes(cp, group, base[10])]
    pts, scs, lengths = [], [], []
    for seg_p, seg_s in cases:
        pts += [pad_pts[i & 1] for i in range(pad)] + seg_p
        scs += [rnd.randrange(cp.r) for _ in range(pad)] + seg_s
        lengths.append(pad + len(seg_p))
    return b"".join(pts), b"".join(sc(v) for v in scs), lengths
