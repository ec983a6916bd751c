"""Inputs of the tests of the GLV lattice split of BN254 G1 (tests/test_g1_glv_host.py, tests/test_g1_glv_gpu.py): the
eigenvalue, the lattice basis and the split as Python integers (recomputed here from p, r, x -- not read from the header),
the scalars on the boundaries of the split, the degenerate pairs the split adds to those of tests/msm_batch_cases.py, the
off-curve point that shows which route ran, and the host build of the split, the chain and the chunk body
(tests/hostmath_glv)."""
import ctypes
import functools
import os
import random
import subprocess
from math import isqrt

from conftest import ROOT
from msm_batch_cases import neg_point, sc
from msm_batch_subgroup_cases import offsets_of
from oracle import pyref as R
from point_sum_cases import distinct_points

CP = R.CURVES["BN254"]
LAM = (36 * CP.x**4 - 1) % CP.r
CHUNKS = (1, 2, 4, 8)
# on y^2 = x^3 + 8, not on the curve: [LAM]T is not (beta, 3), so T with s = LAM shows whether the split ran
T = (1, 3)


@functools.lru_cache(maxsize=None)
def beta():
    """the cube root of unity with (beta x, y) = [LAM]P, from the oracle's own multiplication"""
    P = distinct_points("BN254", 1, 300)[5]
    Q = R.g1_mul(CP, P, LAM)
    b = Q[0] * pow(P[0], -1, CP.p) % CP.p
    assert b != 1 and pow(b, 3, CP.p) == 1 and Q[1] == P[1]
    return b


@functools.lru_cache(maxsize=None)
def basis():
    """(v1, v2) by extended Euclid on (r, LAM): the two rows after the remainder drops below sqrt(r)"""
    rows = [(CP.r, 0), (LAM, 1)]
    while rows[-1][0]:
        q = rows[-2][0] // rows[-1][0]
        rows.append((rows[-2][0] - q * rows[-1][0], rows[-2][1] - q * rows[-1][1]))
    l = max(i for i, v in enumerate(rows) if v[0] >= isqrt(CP.r))
    return (rows[l + 1][0], -rows[l + 1][1]), (rows[l + 2][0], -rows[l + 2][1])


def split(s):
    """(k1, k2) of canonical s as g1_glv_split computes them: the quotients rounded by a 2^256-scaled multiplication"""
    (a1, b1), (a2, b2) = basis()
    c1 = (s * ((abs(b2) << 256) // CP.r) + (1 << 255)) >> 256
    c2 = (s * ((abs(b1) << 256) // CP.r) + (1 << 255)) >> 256
    return s - c1 * a1 - c2 * a2, -c1 * b1 - c2 * b2


@functools.lru_cache(maxsize=None)
def special_scalars():
    """(reduced, unreduced): the named values; for both quotients and the first, middle and last i the scalars around
    ceil(i r / |b|) (where floor(s |b| / r) steps) and around ceil((2 i - 1) r / (2 |b|)) (where the rounded quotient
    steps); values whose k1 or k2 is 0"""
    r = CP.r
    (_, b1), (_, b2) = basis()
    d = R.Drbg("g1_glv/scalars")
    reduced = [0, 1, r - 1, LAM, LAM + 1, LAM - 1, r - LAM, (1 << 64) - 1, (1 << 128) - 1, (1 << 128) + 1]
    for b in (abs(b2), abs(b1)):
        for i in (1, b // 2, b - 1):
            for edge in (-(-i * r // b), -(-(2 * i - 1) * r // (2 * b))):
                reduced += [edge - 1, edge, edge + 1]
    reduced += [7 * LAM % r, d.below(1 << 100), d.below(1 << 100) * LAM % r, d.below(r)]
    assert all(0 <= s < r for s in reduced)
    return tuple(reduced), (r, r + 1, 2 * r + 3, (1 << 256) - 1)


def scalar_rows(mont):
    """[(32 scalar bytes, the multiplier they mean)]: reduced values keep their meaning in both forms; the unreduced ones are
    taken as they are (with scalars_mont they mean s / 2^256 mod r)"""
    reduced, unreduced = special_scalars()
    rinv = pow(1 << 256, -1, CP.r)
    rows = [(R.scalar_to_bytes(s, CP, mont=bool(mont)), s) for s in reduced]
    return rows + [(s.to_bytes(32, "little"), (s * rinv if mont else s) % CP.r) for s in unreduced]


def harness():
    """the ctypes handle of tests/hostmath_glv, built when it is older than the headers"""
    d = os.path.join(ROOT, "tests", "hostmath_glv")
    so = os.path.join(d, "libhostmath_glv.so")
    src = os.path.join(d, "glv.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.glv_available.argtypes = [ci]
    lib.glv_constants.argtypes = [vp] * 6
    lib.glv_constants.restype = None
    lib.glv_phi.argtypes = [vp, vp]
    lib.glv_phi.restype = None
    lib.glv_split.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.glv_split.restype = None
    lib.glv_g1_mul.argtypes = [vp, vp, ci, vp]
    lib.glv_g1_mul.restype = None
    lib.glv_msm_batch.argtypes = [ci, vp, vp, ci, vp, ctypes.c_size_t, vp]
    return lib


def host_split(lib, raw, mont):
    """(k1, k2, s mod r) of the 32 scalar bytes by the compiled split behind fr_canonical"""
    a, b, canon = (ctypes.create_string_buffer(32) for _ in range(3))
    neg = (ctypes.c_int * 2)()
    lib.glv_split(raw, mont, a, b, neg, canon)
    av, bv = int.from_bytes(a.raw, "little"), int.from_bytes(b.raw, "little")
    return (-av if neg[0] else av), (-bv if neg[1] else bv), int.from_bytes(canon.raw, "little")


def host_mul(lib, P, raw, mont):
    """the 64 bytes the chain of k_scalar_mul_endo<Bn254> gives for the affine point P (None: infinity)"""
    out = ctypes.create_string_buffer(64)
    lib.glv_g1_mul(R.g1_to_mont_bytes(CP, P), raw, mont, out)
    return out.raw


def host_batch(lib, P, pts, scs, lengths, mont):
    """(return code, the affine sum of every segment by the split chunk body on the CPU)"""
    out = ctypes.create_string_buffer(max(1, len(lengths)) * 64)
    rc = lib.glv_msm_batch(P, pts, scs, 1 if mont else 0, offsets_of(lengths), len(lengths), out)
    return rc, [out.raw[i * 64 : (i + 1) * 64] for i in range(len(lengths))]


def glv_edge_segments(seed, pad=0):
    """degenerate pairs the lattice split adds, side by side in one chunk (P >= 2), pad pairs in front of each so that they
    also straddle chunk boundaries.  With Q = [LAM]P = phi(P):
      (P, d LAM) beside (Q, d)      k1 = 0 beside k2 = 0: both add the same point at the same loop positions, one through
                                    the endomorphism (the accumulator meets its own table entry: the doubling branch)
      (P, d LAM) beside (-Q, d)     the same pair cancelling to infinity
      (P, d), (Q, d), ([LAM]Q, d)   P + phi P + phi^2 P = infinity
      (P, e + d LAM) beside (Q, r - d)   cancels down to [e]P
      (P, d) / (P, d LAM) alone     k2 = 0 / k1 = 0"""
    rnd = random.Random(seed)
    base = distinct_points("BN254", 1, 300)
    P0 = base[7]
    Q = R.g1_mul(CP, P0, LAM)
    Q2 = R.g1_mul(CP, Q, LAM)
    bP, bQ, bQ2 = (R.g1_to_mont_bytes(CP, p) for p in (P0, Q, Q2))
    d = rnd.randrange(1, 1 << 100)
    e = rnd.randrange(1, 1 << 100)
    r = CP.r
    assert split(d) == (d, 0) and split(d * LAM % r) == (0, d)
    cases = [
        ([bP, bQ], [d * LAM % r, d]),
        ([bQ, bP], [d, d * LAM % r]),
        ([bP, neg_point(CP, 1, bQ)], [d * LAM % r, d]),
        ([bP, bQ, bQ2], [d, d, d]),
        ([bP, bQ, bP, bQ], [d * LAM % r, d, d * LAM % r, d]),
        ([bP, bQ], [(e + d * LAM) % r, r - d]),
        ([bP], [d]),
        ([bP], [d * LAM % r]),
        ([bQ, neg_point(CP, 1, bQ)], [LAM, LAM]),
    ]
    pad_pts = [R.g1_to_mont_bytes(CP, base[9]), R.g1_to_mont_bytes(CP, base[10])]
    pts, scs, lengths = [], [], []
    for seg_p, seg_s in cases:
        pts += [pad_pts[i & 1] for i in range(pad)] + seg_p
        scs += [rnd.randrange(r) for _ in range(pad)] + seg_s
        lengths.append(pad + len(seg_p))
    return b"".join(pts), b"".join(sc(v) for v in scs), lengths
