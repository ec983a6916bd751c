"""K products of m pairs each, for any m (include/mlhip.h: MLHIP_PRODUCT_PAIRS), without a GPU: the groups a product is cut
into, the fold schedule and the slabs, from a g++ build of mathlib_amd/csrc/pairing_products.h (tests/hostmath_products); how
the macro packs and what the six entry points reject before they look for a device; and the three drivers, the binding and the
headers carry the new names."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

PERS = (1, 2, 4)
MS = range(1, 41)
BIT63 = 1 << 63


@pytest.fixture(scope="module")
def pp():
    d = os.path.join(ROOT, "tests", "hostmath_products")
    so = os.path.join(d, "libpairing_products_host.so")
    src = os.path.join(d, "pairing_products_host.cpp")
    deps = [src, os.path.join(ROOT, "mathlib_amd", "csrc", "pairing_products.h"), os.path.join(ROOT, "include", "mlhip.h"),
            os.path.join(ROOT, "include", "mlhip_products.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    lib.pp_group.argtypes = [u32, u32, u64, ctypes.POINTER(u64)]
    lib.pp_fold.argtypes = [u32, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]
    lib.pp_pick.argtypes = [u64, ctypes.c_char_p]
    lib.pp_pick.restype = u64
    lib.pp_slab.argtypes = [u64, u32, u64, u64, u64]
    lib.pp_slab.restype = u64
    for f, t in ((lib.pp_pack_u64, u64), (lib.pp_pack_int, ctypes.c_int), (lib.pp_pack_u32, u32)):
        f.argtypes = [t]
        f.restype = u64
    return lib


def group(pp, m, per, i):
    out = (ctypes.c_uint64 * 4)()
    pp.pp_group(m, per, i, out)
    return out[0], out[1], out[2], out[3]


def test_groups_cover_every_pair_once(pp):
    """every m in 1 .. 40, per in {1, 2, 4}, K = 3 products: g = ceil(m / per); group k g + j starts at pair k m + j per in slot
    j per and holds min(per, m - j per) pairs; together the groups name each pair of each product exactly once, in order"""
    K = 3
    for m in MS:
        for per in PERS:
            g = -(-m // per)
            seen = []
            for i in range(K * g):
                first, count, slot, gg = group(pp, m, per, i)
                if g == 1:
                    # one group per product: the plain layout (miller_group's g = 1 branch; the library never groups m <= 4)
                    assert (first, count, slot) == (i * m, m, 0), (m, per, i)
                    seen += list(range(first, first + count))
                    continue
                k, j = divmod(i, g)
                assert gg == g
                assert first == k * m + j * per and slot == j * per, (m, per, i)
                assert count == min(per, m - j * per) and 1 <= count <= per, (m, per, i)
                seen += list(range(first, first + count))
            assert seen == list(range(K * m)), (m, per)
            tail = m - (g - 1) * per
            assert group(pp, m, per, g - 1)[1] == (m if g == 1 else tail)


def test_one_group_reproduces_the_plain_addressing(pp):
    """g = 1 (the calls of at most four pairs): group i is product i, ppp pairs from i ppp -- also for an index past 2^32"""
    for ppp in (1, 2, 3, 4):
        for i in (0, 1, 63, 64, 65535, (1 << 32) + 5):
            assert group(pp, ppp, 0, i) == (i * ppp, ppp, 0, 1)


PRIMES = []


def primes(n):
    c = PRIMES[-1] + 1 if PRIMES else 2
    while len(PRIMES) < n:
        if all(c % p for p in PRIMES if p * p <= c):
            PRIMES.append(c)
        c += 1
    return PRIMES[:n]


def test_fold_uses_every_partial_once_and_leaves_the_product_at_k(pp):
    """the fold replayed on distinct primes modulo the word-sized prime 2^61 - 1, K = 5 products of g values for every g that
    m in 1 .. 40 and per in {1, 2, 4} give: out[k] is the product of product k's g values, every value is read as an operand
    for the first time exactly once (a slot read again holds an earlier pass's product), and the number of passes is
    ceil(log2 g)"""
    mod, K = (1 << 61) - 1, 5
    for g in sorted({-(-m // per) for m in MS for per in PERS}):
        vals = primes(K * g)
        part = (ctypes.c_uint64 * (K * g))(*vals)
        out = (ctypes.c_uint64 * K)(*([0xDEAD] * K))
        reads = (ctypes.c_uint32 * (K * g))()
        passes = pp.pp_fold(g, K, mod, part, out, reads)
        if g == 1:
            assert passes == 0 and list(out) == [0xDEAD] * K  # nothing to fold: the Miller kernel wrote out[k] itself
            continue
        assert passes == (g - 1).bit_length(), g
        for k in range(K):
            want = 1
            for v in vals[k * g : (k + 1) * g]:
                want = want * v % mod
            assert out[k] == want, (g, k)
        # g values and g - 1 products per product: 2 (g - 1) operand reads, every slot at least once
        assert sum(reads) == 2 * K * (g - 1) and min(reads) >= 1, g


def test_group_pick_and_slabs(pp):
    assert [pp.pp_pick(1 << 10, f) for f in (b"1", b"2", b"4")] == [1, 2, 4]
    for junk in (None, b"", b"3", b"8", b"0", b"44", b"x"):
        assert pp.pp_pick((1 << 17) - 1, junk) == 1 and pp.pp_pick(1 << 17, junk) == 4
    gt = 576
    cap = 1 << 30
    assert pp.pp_slab(13, 5, gt, 256, cap) == 13  # everything fits: one slab
    fit = (cap - 256) // gt // 5
    assert pp.pp_slab(10 * fit, 5, gt, 256, cap) == fit and fit * 5 * gt + 256 <= cap < (fit + 1) * 5 * gt + 256
    assert pp.pp_slab(7, (cap // gt) + 1, gt, 0, cap) == 0  # one product's partials alone exceed the cap
    assert pp.pp_slab(7, cap // gt, gt, 0, cap) == 1
    assert pp.pp_slab(7, 3, gt, 4096, 4096 + 7 * gt) == 2  # a small cap: slabs of two products


def test_macro_packs_and_the_entry_points_reject(pp, mlhip):
    """bit 63 and m in the low 32 bits; m = 0, a negative m and m >= 2^32 pack to bit 63 alone, which all six entry points
    reject (as they reject bits between 32 and 62) before they look at a buffer or for a device; a plain value above 4 stays
    MLHIP_EINVAL; the binding packs as the macro does"""
    for m in (1, 4, 5, 9, 40, (1 << 32) - 1):
        assert pp.pp_pack_u64(m) == BIT63 | m == mlhip.product_pairs(m)
    for m in (0, 1 << 32, (1 << 32) + 9, 1 << 40, BIT63 | 5):
        assert pp.pp_pack_u64(m) == BIT63 == mlhip.product_pairs(m)
    assert pp.pp_pack_int(-1) == BIT63 == mlhip.product_pairs(-1) and pp.pp_pack_int(17) == BIT63 | 17
    assert pp.pp_pack_u32(0) == BIT63 and pp.pp_pack_u32(0xFFFFFFFF) == BIT63 | 0xFFFFFFFF
    lib = mlhip.load()
    out = ctypes.create_string_buffer(b"\xA5" * 8, 8)
    bad = [BIT63, BIT63 | (1 << 32), BIT63 | (1 << 40) | 9, 5, 9, 0]
    for ppp in bad:
        assert lib.mlhip_miller_loop(1, b"x", b"y", ppp, 1, out) == mlhip.EINVAL, hex(ppp)
        assert lib.mlhip_miller_loop_device(1, b"x", b"y", ppp, 1, out, None) == mlhip.EINVAL, hex(ppp)
        assert b"1..4" in lib.mlhip_last_error() or b"MLHIP_PRODUCT_PAIRS" in lib.mlhip_last_error()
    for fn in (lib.mlhip_miller_loop_prepared, lib.mlhip_pairing_prepared):
        assert fn(None, b"x", None, BIT63 | 9, 1, out) == mlhip.EINVAL  # null handle
    for fn in (lib.mlhip_miller_loop_prepared_device, lib.mlhip_pairing_prepared_device):
        assert fn(None, b"x", None, BIT63 | 9, 1, out, None) == mlhip.EINVAL
    # an empty batch is nothing to do, an overflowing one is rejected before anything is launched (host form: before the
    # library looks for a device)
    assert lib.mlhip_miller_loop(1, b"x", b"y", BIT63 | 9, 0, out) == 0
    assert lib.mlhip_miller_loop(1, b"x", b"y", BIT63 | 9, 1 << 62, out) == mlhip.EINVAL
    assert lib.mlhip_miller_loop(1, b"x", b"y", BIT63 | 0xFFFFFFFF, 1 << 40, out) == mlhip.EINVAL
    assert lib.mlhip_miller_loop(1, None, b"y", BIT63 | 9, 1, out) == mlhip.EINVAL
    assert lib.mlhip_miller_loop(1, b"x", b"y", BIT63 | 9, 1, None) == mlhip.EINVAL
    assert lib.mlhip_miller_loop(7, b"x", b"y", BIT63 | 9, 1, out) == mlhip.EINVAL  # unknown curve
    assert out.raw == b"\xA5" * 8


def test_drivers_binding_and_headers_carry_the_names(mlhip):
    """the exported ABI has not grown: the length travels in pairs_per_product (MLHIP_PRODUCT_PAIRS), include/mlhip_products.h
    and the binding give the six functions over it, and the three drivers have the methods"""
    from mathlib_amd import build
    from mathlib_amd.driver import Curve, G2Prepared

    fns = build.abi_functions()
    names = ("mlhip_miller_loop_products", "mlhip_miller_loop_products_device", "mlhip_miller_loop_prepared_products",
             "mlhip_miller_loop_prepared_products_device", "mlhip_pairing_prepared_products", "mlhip_pairing_prepared_products_device")
    assert sorted(fns) == sorted(mlhip.SYMBOLS) and len(fns) == 77 and not set(names) & set(fns)
    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert "#define MLHIP_PRODUCT_PAIRS(m)" in hdr and "mlhip_products.h" in hdr and "products of any length" in hdr
    assert "(pairs_per_product <= 4)" not in hdr
    inl = open(os.path.join(ROOT, "include", "mlhip_products.h")).read()
    for fn in names:
        decl = re.search(r"^static inline int %s\(([^)]*)\)" % fn, inl, re.M | re.S)
        args = " ".join(decl.group(1).split()) if decl else ""
        assert "size_t m, size_t n_products" in args, fn
        assert ("void* stream" in args) == fn.endswith("_device"), fn
        assert callable(getattr(mlhip, fn))
    assert inl.count("MLHIP_PRODUCT_PAIRS(m)") >= 6
    # taken apart in api_pairing.hip's unpack_pairs and nowhere else in the library
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".inc")) and "unpack_pairs(" in open(os.path.join(csrc, f)).read())
    assert users == ["api_pairing.hip"]
    hpp = open(os.path.join(ROOT, "include", "mlhip_driver.hpp")).read()
    go = open(os.path.join(ROOT, "go", "driver", "hip", "hip.go")).read()
    for meth in ("MillerLoopProducts", "PairingProducts"):
        assert callable(getattr(Curve, meth))
        assert re.search(r"std::vector<Gt> %s\(const std::vector<std::vector<G2>>& g2, const std::vector<std::vector<G1>>& g1\) const" % meth, hpp), meth
        assert re.search(r"^func \(c \*Curve\) %s\(g2s \[\]\[\]driver\.G2, g1s \[\]\[\]driver\.G1\) \[\]driver\.Gt" % meth, go, re.M), meth
    for meth in ("MillerLoopBatch", "PairingBatch"):
        assert callable(getattr(G2Prepared, meth))
        assert re.search(r"^func \(p \*G2Prepared\) %s\(g1s \[\]\[\]driver\.G1, index \[\]uint32\) \[\]driver\.Gt" % meth, go, re.M), meth
    assert "C.mlhip_miller_loop_products(" in go and "C.mlhip_pairing_prepared_products(" in go and '#include "mlhip_products.h"' in go
    assert "mlhip_miller_loop_products(" in hpp and "mlhip_pairing_prepared_products(" in hpp and '#include "mlhip_products.h"' in hpp
    assert callable(mlhip.miller_loop_products) and callable(mlhip.g2_prepared_products)
