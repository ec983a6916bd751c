"""Short-scalar MSM plans (mlhip_msm_plan_create_bits / mlhip_msm_bits) without a GPU: the width rule, the layout over
bits + 1 bits, the masked canonical scalar, the digits and a whole MSM replayed in the kernels' order, from a g++ build of
the kernels' headers (tests/hostmath_bits), against oracle.pyref on the masked scalars; and the three drivers, the binding
and the header carry the new names."""
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


@pytest.fixture(scope="module")
def mb():
    d = os.path.join(ROOT, "tests", "hostmath_bits")
    so = os.path.join(d, "libmsm_bits_host.so")
    src = os.path.join(d, "msm_bits_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMLHIP_HOST_USE_DEVICE_PATH", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.mb_layout.argtypes = [ci, ci, ctypes.POINTER(ci)]
    lib.mb_shifts.argtypes = [ci, ci, ctypes.POINTER(ci), ci]
    lib.mb_digits.argtypes = [ci, vp, ci, ci, ci, ctypes.POINTER(ctypes.c_uint32), ci]
    lib.mb_masked.argtypes = [ci, vp, ci, ci, vp]
    lib.mb_msm.argtypes = [ci, vp, vp, ci, ctypes.c_size_t, ci, ci, vp]
    return lib


def layout(mb, bits, c):
    """(W, [offsets], [widths]) of the balanced layout over bits + 1 bits at width c, as the kernels compute it"""
    out = (ctypes.c_int * 3)()
    mb.mb_layout(bits, c, out)
    W, base, rem = out[0], out[1], out[2]
    widths = [base + (1 if w < rem else 0) for w in range(W)]
    offs = [w * base + min(w, rem) for w in range(W)]
    return W, offs, widths


def test_width_rule_and_layout(mb):
    """every curve's range of bits, every c: W = ceil((bits + 1) / c), c' = ceil((bits + 1) / W) <= c, the layout under c'
    has the same W, widths that differ by at most one, sum to bits + 1 and have c' as their maximum; the host tail's shifts
    are the differences of the offsets"""
    for name in CURVES:
        assert mb.mb_fr_bits(R.CURVES[name].curve_id) == FR_BITS[name]
    for bits in range(1, max(FR_BITS.values()) + 1):
        for c in range(4, 21):
            B = bits + 1
            W = -(-B // c)
            cp_ = -(-B // W)
            assert mb.mb_effective_c(bits, c) == cp_ <= c, (bits, c)
            assert layout(mb, bits, c)[0] == W
            W2, offs, widths = layout(mb, bits, cp_)
            assert W2 == W, (bits, c, cp_)
            assert max(widths) - min(widths) <= 1 and sum(widths) == B and max(widths) == cp_, (bits, c, widths)
            assert offs[0] == 0 and all(offs[w + 1] == offs[w] + widths[w] for w in range(W - 1))
            assert mb.mb_effective_c(bits, cp_) == cp_  # c' is a fixed point: storing it as the plan's c changes nothing
            down = (ctypes.c_int * 80)()
            assert mb.mb_shifts(bits, cp_, down, 80) == W
            assert down[0] == 0 and [down[w] for w in range(1, W)] == [offs[w] - offs[w - 1] for w in range(1, W)]
            assert sum(down[w] for w in range(W)) == offs[-1] <= bits


BITS = (1, 2, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
WIDTHS = (4, 8, 13, 16, 20)


def digit_value(out, W, offs, widths):
    tot = 0
    for w in range(W):
        d = out[w]
        if d:
            mag, neg = d >> 1, d & 1
            assert 1 <= mag <= 1 << (widths[w] - 1), (w, mag, widths[w])
            tot += (-mag if neg else mag) << offs[w]
    return tot


@pytest.mark.parametrize("name", CURVES)
def test_digits_of_masked_scalars(mb, name):
    """sum_w d_w 2^off(w) = (s mod r) mod 2^bits with |d_w| <= 2^(width(w) - 1), for plain and Montgomery inputs: the edge
    values, all-ones in each single window, r - 1, 2^256 - 1 and 200 random 256-bit values"""
    cp = R.CURVES[name]
    rnd = random.Random("msm-bits/digits/" + name)
    randoms = [rnd.getrandbits(256) for _ in range(200)]
    for bits in BITS + (FR_BITS[name] - 1, FR_BITS[name]):
        for c in WIDTHS:
            ce = max(4, mb.mb_effective_c(bits, c))  # what the plan stores (api_msm.hip: never below 4)
            W, offs, widths = layout(mb, bits, ce)
            assert W == -(-(bits + 1) // c)
            cases = [0, 1, (1 << bits) - 1, 1 << (bits - 1), cp.r - 1, (1 << 256) - 1]
            cases += [(((1 << widths[w]) - 1) << offs[w]) & ((1 << bits) - 1) for w in range(W)]
            for s in cases + randoms:
                want = (s % cp.r) % (1 << bits)
                for mont in (0, 1):
                    # (a Montgomery row holds s R mod r: only canonical values have one)
                    enc = ((s % cp.r) * (1 << 256) % cp.r) if mont else s
                    out = (ctypes.c_uint32 * 80)()
                    assert mb.mb_digits(cp.curve_id, enc.to_bytes(32, "little"), mont, ce, bits, out, 80) == W
                    assert digit_value(out, W, offs, widths) == want, (name, bits, c, hex(s), mont)
                    m = ctypes.create_string_buffer(32)
                    assert mb.mb_masked(cp.curve_id, enc.to_bytes(32, "little"), mont, bits, m) == 0
                    assert int.from_bytes(m.raw, "little") == want


@pytest.mark.parametrize("name", CURVES)
def test_full_width_digits_are_the_existing_ones(mb, hostmath, name):
    """bits = fr_bits: the same digits as the full-width body the existing host-math library exports (hm_digits)"""
    cp = R.CURVES[name]
    rnd = random.Random("msm-bits/full/" + name)
    for c in (4, 8, 13, 15, 16, 17, 20):
        for s in [0, 1, cp.r - 1, (1 << 256) - 1] + [rnd.getrandbits(256) for _ in range(40)]:
            for mont in (0, 1):
                enc = ((s % cp.r) * (1 << 256) % cp.r) if mont else s
                a = (ctypes.c_uint32 * 80)()
                b = (ctypes.c_uint32 * 80)()
                W = hostmath.hm_digits(cp.curve_id, enc.to_bytes(32, "little"), mont, c, a, 80)
                assert W > 0 and mb.mb_digits(cp.curve_id, enc.to_bytes(32, "little"), mont, c, FR_BITS[name], b, 80) == W
                assert list(a[:W]) == list(b[:W]), (name, c, hex(s), mont)


N_REPLAY = 40


def replay_inputs(name):
    cp = R.CURVES[name]
    d = R.Drbg("msm-bits/replay/" + name)
    pts = [R.random_g1(cp, d) for _ in range(N_REPLAY)]
    pts[5] = None  # an infinity
    pts[9] = pts[3]  # a repeated point
    pts[21] = R.g1_neg(cp, pts[20])  # P beside -P
    rnd = random.Random("msm-bits/replay/" + name)
    sc = [rnd.getrandbits(256) for _ in range(N_REPLAY)]
    sc[0], sc[1], sc[2], sc[4] = 0, 1, cp.r - 1, (1 << 256) - 1
    sc[21] = sc[20]  # the pair cancels in every window
    return cp, pts, sc


@pytest.mark.parametrize("name", CURVES)
def test_replayed_msm_matches_pyref_on_masked_scalars(mb, name):
    """digits -> buckets -> window sums -> the host tail's Horner pass over the short layout, for 40 points with an infinity, a
    repeated point and P beside -P: oracle.pyref's MSM over (s mod r) mod 2^bits"""
    cp, pts, sc = replay_inputs(name)
    raw = b"".join(R.g1_to_mont_bytes(cp, p) for p in pts)
    for bits in (1, 15, 16, 17, 129):
        top = (1 << bits) - 1
        scb = list(sc)
        scb[6], scb[7] = top, 1 << (bits - 1)
        want = R.g1_to_mont_bytes(cp, R.g1_msm(cp, pts, [(s % cp.r) & top for s in scb]))
        buf = b"".join(s.to_bytes(32, "little") for s in scb)
        for c in (4, 8, 16):
            ce = max(4, mb.mb_effective_c(bits, c))
            out = ctypes.create_string_buffer(2 * cp.fp_bytes)
            assert mb.mb_msm(cp.curve_id, raw, buf, 0, N_REPLAY, ce, bits, out) == -(-(bits + 1) // c)
            assert out.raw == want, (name, bits, c)


def test_drivers_binding_and_headers_carry_the_names(mlhip):
    """the exported ABI has not grown: the width travels in window_c (MLHIP_WINDOW_BITS), include/mlhip_bits.h and the binding
    give the three functions over it, and the three drivers have the two methods"""
    from mathlib_amd import build
    from mathlib_amd.driver import Curve

    fns = build.abi_functions()
    names = ("mlhip_msm_plan_create_bits", "mlhip_msm_plan_scalar_bits", "mlhip_msm_bits")
    assert sorted(fns) == sorted(mlhip.SYMBOLS) and not set(names) & set(fns)
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert "#define MLHIP_WINDOW_BITS(window_c, scalar_bits)" in hdr and "mlhip_bits.h" in hdr
    inl = open(os.path.join(ROOT, "include", "mlhip_bits.h")).read()
    for fn in names:
        decl = re.search(r"^static inline int %s\(([^)]*)\)" % fn, inl, re.M | re.S)
        assert decl and "stream" not in decl.group(1), fn  # rides the existing launch entry points: no stream of its own
        assert callable(getattr(mlhip, fn))
    # the binding packs as the macro does: width in the low byte, scalar width above, out-of-range values made invalid
    assert mlhip.window_bits(16, 64) == 16 | (64 << 8) and mlhip.window_bits(0, 0) == 0 and mlhip.window_bits(13, 256) == 13 | (256 << 8)
    assert mlhip.window_bits(16, -1) >> 8 == 0x3FF == mlhip.window_bits(16, 257) >> 8 and mlhip.window_bits(300, 64) & 0xFF == 0xFF
    hpp = open(os.path.join(ROOT, "include", "mlhip_driver.hpp")).read()
    go = open(os.path.join(ROOT, "go", "driver", "hip", "hip.go")).read()
    for g, meth in ((1, "MultiScalarMulShort"), (2, "MultiScalarMulG2Short")):
        assert callable(getattr(Curve, meth))
        assert re.search(r"\bG%d %s\(const std::vector<G%d>& a, const std::vector<Zr>& b, int bits\) const" % (g, meth, g), hpp), meth
        assert re.search(r"^func \(c \*Curve\) %s\(a \[\]driver\.G%d, b \[\]driver\.Zr, bits int\) driver\.G%d" % (meth, g, g), go, re.M), meth
    assert "C.mlhip_msm_bits(" in go and "mlhip_msm_bits(" in hpp and '#include "mlhip_bits.h"' in go and '#include "mlhip_bits.h"' in hpp
    assert callable(mlhip.msm_bits) and callable(mlhip.MsmPlan.scalar_bits)
