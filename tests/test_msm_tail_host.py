"""The tail kernel of a device-result MSM plan without a GPU: the MLHIP_HD bodies of mathlib_amd/csrc/msm_tail.h replayed lane
by lane from a g++ build (tests/hostmath_tail), on random and on degenerate partial sums, against what a host-result plan
computes from the same bytes (host_tail_window + horner_jac + xyzz_to_affine) and against oracle.pyref; and the flag, the
binding, the header and the symbol table.  Fails without the feature: there is no msm_tail.h to build."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT
from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]
FR_BITS = {"BN254": 254, "BLS12-381": 255, "BLS12-377": 253}
G1, G2 = 1, 2


@pytest.fixture(scope="module")
def mt():
    d = os.path.join(ROOT, "tests", "hostmath_tail")
    so = os.path.join(d, "libmsm_tail_host.so")
    src = os.path.join(d, "msm_tail_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "mlhip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    newest = max(os.path.getmtime(f) for f in deps)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci, ip = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    lib.mt_shifts.argtypes = [ci, ci, ip, ci]
    lib.mt_scaled.argtypes = [ci, ci, vp, vp, vp]
    lib.mt_to_affine.argtypes = [ci, ci, vp, vp]
    lib.mt_kernel.argtypes = [ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ip, vp, vp]
    lib.mt_host.argtypes = [ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]
    return lib


class Group:
    """one curve's G1 or G2 through oracle.pyref"""

    def __init__(self, name, group):
        self.cp = R.CURVES[name]
        self.name, self.group = name, group
        g1 = group == G1
        self.ptsz = (2 if g1 else 4) * self.cp.fp_bytes
        self.elem = self.ptsz // 2
        self.to_bytes = (R.g1_to_mont_bytes if g1 else R.g2_to_mont_bytes)
        self.from_bytes = (R.g1_from_mont_bytes if g1 else R.g2_from_mont_bytes)
        self.add = (R.g1_add if g1 else R.g2_add)
        self.neg = (R.g1_neg if g1 else R.g2_neg)
        self.mul = (R.g1_mul_unreduced if g1 else R.g2_mul_unreduced)
        self.rand = (R.random_g1 if g1 else R.random_g2)

    def b(self, P):
        return self.to_bytes(self.cp, P)


_POOLS = {}


def pool(mt, name, group):
    """(Group, [affine points], [XYZZ bytes of each under some non-trivial representative], XYZZ bytes of infinity)"""
    key = (name, group)
    if key not in _POOLS:
        g = Group(name, group)
        d = R.Drbg("msm-tail/pool/%s/%d" % (name, group))
        pts = [g.rand(g.cp, d) for _ in range(12)]
        lam = [g.b(g.rand(g.cp, d))[: g.elem] for _ in range(12)]  # the x coordinate of a point: some field element
        inf = xyzz_of(mt, g, None, lam[0])
        _POOLS[key] = (g, pts, [xyzz_of(mt, g, P, l) for P, l in zip(pts, lam)], inf, lam)
    return _POOLS[key]


def xyzz_of(mt, g, P, lam):
    out = ctypes.create_string_buffer(2 * g.ptsz)
    assert mt.mt_scaled(g.cp.curve_id, g.group, g.b(P), lam, out) == 0
    return out.raw


def geometry(mt, name, bits, c):
    """(c', W, nsel, nb, lgL, down) as api_msm.hip: plan_create_ex lays a plain plan out"""
    fr = FR_BITS[name]
    bits = fr if bits >= fr else bits
    if bits < fr:
        W0 = -(-(bits + 1) // c)
        c = max(4, -(-(bits + 1) // W0))
    W = -(-(bits + 1) // c)
    M = 1 << (c - 1)
    lgL = 4 if (M >= 256 and W * M >= 1 << 17) else 3
    nb = c - 1 - lgL
    down = (ctypes.c_int * 64)()
    assert mt.mt_shifts(bits, c, down, 64) == W <= mt.mt_max_windows()
    return bits, c, W, 4 + nb, nb, lgL, down


def run_both(mt, g, entries, W, nsel, nb, lgL, first, horner, empty, bits, c, down):
    """(kernel replay, host tail), each (xyzz bytes, affine bytes); the affine points must be the same bytes, and each XYZZ
    value must normalise to its affine point"""
    buf = b"".join(entries)
    res = []
    for which in ("kernel", "host"):
        x = ctypes.create_string_buffer(2 * g.ptsz)
        a = ctypes.create_string_buffer(b"\xAA" * g.ptsz, g.ptsz)
        if which == "kernel":
            rc = mt.mt_kernel(g.cp.curve_id, g.group, buf, W, nsel, nb, lgL, first, horner, empty, down, x, a)
        else:
            rc = mt.mt_host(g.cp.curve_id, g.group, buf, W, nsel, nb, lgL, first, horner, empty, bits, c, x, a)
        assert rc == 0
        n = ctypes.create_string_buffer(g.ptsz)
        mt.mt_to_affine(g.cp.curve_id, g.group, x.raw, n)
        assert n.raw == a.raw, which
        res.append((x.raw, a.raw))
    assert res[0][1] == res[1][1]
    assert res[0][0] == res[1][0]  # the same operations on the same bytes: the XYZZ values agree too
    return res[0][1]


def expected(g, chosen, W, nsel, nb, lgL, offs):
    """sum_w 2^off(w) (sum_{q<4} e[w][q] + 2^lgL sum_k 2^k e[w][4+k]) in pyref, from the affine points behind the entries"""
    tot = None
    for w in range(W):
        V = None
        for q in range(4 + nb):
            P = chosen[w * nsel + q]
            if P is not None:
                V = g.add(g.cp, V, P if q < 4 else g.mul(g.cp, P, 1 << (lgL + q - 4)))
        if V is not None:
            tot = g.add(g.cp, tot, g.mul(g.cp, V, 1 << offs[w]))
    return g.b(tot)


GROUPS = [(n, G1) for n in CURVES] + [(n, G2) for n in CURVES]
GRID = [(b, c) for b in (33, 128, 256) for c in (4, 8, 13, 16)]


@pytest.mark.parametrize("name,group", GROUPS)
def test_random_partial_sums(mt, name, group):
    """every (bits, c) of {33, 128, fr_bits} x {4, 8, 13, 16}: entries drawn from 12 points in non-trivial representatives, a
    fifth of them at infinity, one whole window at infinity; the first geometry of each width is also checked against pyref"""
    g, pts, xs, inf, _ = pool(mt, name, group)
    rnd = random.Random("msm-tail/random/%s/%d" % (name, group))
    for bits_in, c_in in GRID:
        bits, c, W, nsel, nb, lgL, down = geometry(mt, name, bits_in, c_in)
        idx = [rnd.randrange(-3, 12) for _ in range(W * nsel)]
        dead = rnd.randrange(W)
        for q in range(nsel):
            idx[dead * nsel + q] = -1
        entries = [xs[i] if i >= 0 else inf for i in idx]
        got = run_both(mt, g, entries, W, nsel, nb, lgL, 0, 1, 0, bits, c, down)
        if bits_in == 33:  # (few windows: pyref's scalar multiplications stay cheap)
            offs = [sum(down[1 : w + 1]) for w in range(W)]
            assert got == expected(g, [pts[i] if i >= 0 else None for i in idx], W, nsel, nb, lgL, offs), (name, group, bits, c)


@pytest.mark.parametrize("name,group", GROUPS)
def test_degenerate_partial_sums(mt, name, group):
    """all entries at infinity; an empty MSM; the top windows empty; a window sum EQUAL to the running Horner value (the
    Jacobian addition doubles), OPPOSITE to it (infinity, and the pass goes on from there), equal and opposite entries
    inside one window"""
    g, pts, xs, inf, lam = pool(mt, name, group)
    zero = bytes(g.ptsz)
    for bits_in, c_in in ((256, 16), (256, 8), (128, 13), (33, 4)):
        bits, c, W, nsel, nb, lgL, down = geometry(mt, name, bits_in, c_in)
        blank = [inf] * (W * nsel)
        args = (W, nsel, nb, lgL, 0, 1)
        assert run_both(mt, g, blank, *args, 0, bits, c, down) == zero
        garbage = [xs[3]] * (W * nsel)  # an empty MSM reads nothing
        x = ctypes.create_string_buffer(2 * g.ptsz)
        a = ctypes.create_string_buffer(b"\xAA" * g.ptsz, g.ptsz)
        assert mt.mt_kernel(g.cp.curve_id, g.group, b"".join(garbage), W, nsel, nb, lgL, 0, 1, 1, down, x, a) == 0
        assert a.raw == zero and x.raw == inf
        # only window 0 populated
        e = list(blank)
        e[0], e[5] = xs[1], xs[2]
        want = g.b(g.add(g.cp, pts[1], g.mul(g.cp, pts[2], 1 << (lgL + 1))))
        assert run_both(mt, g, e, *args, 0, bits, c, down) == want
        # V[top] = P, then down[top] doublings, then V[top - 1] = +-[2^down[top]] P; a third window below goes on from there
        top = W - 1
        P = pts[4]
        Q = g.mul(g.cp, P, 1 << down[top])
        offs = [sum(down[1 : w + 1]) for w in range(W)]
        for sign in (1, -1):
            Qs = Q if sign > 0 else g.neg(g.cp, Q)
            e = list(blank)
            e[top * nsel + 0] = xs[4]
            e[(top - 1) * nsel + 1] = xyzz_of(mt, g, Qs, lam[5])
            chosen = [None] * (W * nsel)
            chosen[top * nsel + 0], chosen[(top - 1) * nsel + 1] = P, Qs
            got = run_both(mt, g, e, *args, 0, bits, c, down)
            assert got == expected(g, chosen, W, nsel, nb, lgL, offs)
            if sign < 0:
                assert got == zero
            if W >= 3:
                e[(top - 2) * nsel + 2] = xs[6]
                chosen[(top - 2) * nsel + 2] = pts[6]
                got = run_both(mt, g, e, *args, 0, bits, c, down)
                assert got == expected(g, chosen, W, nsel, nb, lgL, offs)
                if sign < 0:
                    assert got == g.b(g.mul(g.cp, pts[6], 1 << offs[top - 2]))
        # inside one window: P + P (the XYZZ addition doubles), then - 2 P in another representative (it cancels)
        e = list(blank)
        e[0], e[1] = xs[7], xyzz_of(mt, g, pts[7], lam[8])
        assert run_both(mt, g, e, *args, 0, bits, c, down) == g.b(g.mul(g.cp, pts[7], 2))
        e[2] = xyzz_of(mt, g, g.neg(g.cp, g.mul(g.cp, pts[7], 2)), lam[9])
        assert run_both(mt, g, e, *args, 0, bits, c, down) == zero


@pytest.mark.parametrize("name,group", GROUPS)
def test_fold_forms(mt, name, group):
    """a folded plan's tail is one window and no Horner pass: the fold_nsel2 combined entries behind the W x nsel ones (20-bit
    digits: 16 groups of 2^15 buckets, nb2 = nb + lg W), or the only group's own entries (13-bit digits: one group)"""
    g, pts, xs, inf, _ = pool(mt, name, group)
    rnd = random.Random("msm-tail/fold/%s/%d" % (name, group))
    none = (ctypes.c_int * 64)()
    for Wg, nb, lgL in ((16, 11, 4), (1, 9, 3)):
        nsel = 4 + nb
        lgW = Wg.bit_length() - 1
        nsel2 = (4 + nb + lgW) if Wg > 1 else 0
        first = Wg * nsel if nsel2 else 0
        nb2 = nsel2 - 4 if nsel2 else nb
        idx = [rnd.randrange(-2, 12) for _ in range(Wg * nsel + nsel2)]
        entries = [xs[i] if i >= 0 else inf for i in idx]
        got = run_both(mt, g, entries, 1, nsel, nb2, lgL, first, 0, 0, FR_BITS[name], 16, none)
        chosen = [pts[i] if i >= 0 else None for i in idx[first : first + 4 + nb2]]
        assert got == expected(g, chosen, 1, 4 + nb2, nb2, lgL, [0]), (name, group, Wg)
        assert run_both(mt, g, [inf] * len(entries), 1, nsel, nb2, lgL, first, 0, 0, FR_BITS[name], 16, none) == bytes(g.ptsz)


def test_flag_macro_binding_and_unpacking(mt, mlhip):
    """MLHIP_WINDOW_DEVICE_RESULT is bit 20 in the header, the g++ build and the binding; it survives beside
    MLHIP_WINDOW_BITS, which never sets a bit above 17, and comes off without disturbing c and bits for every legal pair"""
    flag = mt.mt_flag()
    assert flag == 1 << 20 == mlhip.WINDOW_DEVICE_RESULT
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert re.search(r"^#define MLHIP_WINDOW_DEVICE_RESULT \(1 << 20\)", hdr, re.M)
    for c in list(range(0, 21)) + [255, 300, -1]:
        for bits in list(range(0, 257)) + [-1, 257, 1000]:
            packed = mt.mt_window_bits(c, bits)
            assert packed == mlhip.window_bits(c, bits) and packed < 1 << 18 and not packed & flag
            both = packed | flag
            assert both > 0 and both & flag and both & ~flag == packed
            if 0 <= c <= 20 and 0 <= bits <= 256:  # the legal pairs: what unpack_window (api_msm.hip) reads back
                assert (both & ~flag) & 0xFF == c and (both & ~flag) >> 8 == bits
    # without the flag taken off, the scalar width a packed value unpacks to is out of range: every entry point that does
    # not know the flag rejects it
    assert (flag | 16) >> 8 > 256


def test_header_binding_and_symbol_table(mlhip):
    """the dynamic symbol table still has its 77 functions and none of the new names; include/mlhip_device_result.h and the
    binding carry the six functions; the phrases tests/stream_order_cases.py quotes from mlhip.h still stand"""
    from mathlib_amd import build

    fns = build.abi_functions()
    names = ("mlhip_msm_plan_create_device_result", "mlhip_msm_plan_is_device_result", "mlhip_msm_run_device",
             "mlhip_msm_finish_device", "mlhip_bases_create_device_result", "mlhip_bases_msm_to_device")
    assert len(fns) == 77 == len(mlhip.SYMBOLS) and sorted(fns) == sorted(mlhip.SYMBOLS) and not set(names) & set(fns)
    inl = open(os.path.join(ROOT, "include", "mlhip_device_result.h")).read()
    for fn in names:
        assert re.search(r"^static inline int %s\(" % fn, inl, re.M), fn
        assert callable(getattr(mlhip, fn))
    assert callable(mlhip.MsmPlan.run_device) and callable(mlhip.MsmPlan.finish_device) and callable(mlhip.MsmPlan.is_device_result)
    assert callable(mlhip.bases_create_device_result)
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    flat = " ".join(hdr.split())  # (as tests/test_stream_order_table.py reads it)
    assert "device results" in hdr and "mlhip_device_result.h" in hdr
    for phrase in ("the call returns after the result is there", "as in mlhip_msm_run", "enqueues the kernels and the", "Finish each",
                   "enqueue their kernels on `stream` and return", "in order on `stream`"):
        assert phrase in flat, phrase
    assert "Go shim holds no device pointers" in " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
