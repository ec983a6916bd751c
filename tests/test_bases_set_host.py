"""Sets of resident-bases handles without a GPU (include/mlhip.h, "sets of handles"): the class rule of
mathlib_amd/csrc/msm_set.h compiled with g++ (tests/hostmath_set) and asked through ctypes, the way api_bases.hip asks it;
the argument rules of mlhip_bases_set_create that need no device; and the header, the inline header and the bindings that
carry the two new names over the unchanged symbol table."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def hset():
    d = os.path.join(ROOT, "tests", "hostmath_set")
    so = os.path.join(d, "libset_host.so")
    src = os.path.join(d, "set_host.cpp")
    csrc = os.path.join(ROOT, "mathlib_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("msm_set.h", "msm_segments.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hset_classes.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.hset_class_tiles.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_size_t]
    lib.hset_share.argtypes = [ctypes.c_size_t, ctypes.c_int]
    lib.hset_share_min_n.argtypes = [ctypes.c_int]
    lib.hset_share_min_n.restype = ctypes.c_longlong
    return lib


FIELDS = ("fold", "c", "Wd", "fold_tile", "W", "M", "bits", "can_train")
FOLDED = dict(fold=1, c=20, Wd=13, fold_tile=1 << 20, W=16, M=32768, bits=255, can_train=1)
PLAIN = dict(fold=0, c=16, Wd=16, fold_tile=0, W=16, M=32768, bits=255, can_train=1)


def classes(hset, members):
    flat = [int(m[f]) for m in members for f in FIELDS]
    geo = (ctypes.c_longlong * len(flat))(*flat)
    cls = (ctypes.c_int * len(members))()
    n = hset.hset_classes(geo, len(members), cls)
    return n, list(cls)


def test_equal_geometries_form_one_class_whatever_the_group(hset):
    """the geometry does not name the group: G1 and G2 members of equal geometry read the same lists"""
    assert hset.hset_max_members() == 4
    for g in (FOLDED, PLAIN):
        for k in (1, 2, 3, 4):
            assert classes(hset, [dict(g)] * k) == (1, [0] * k)


@pytest.mark.parametrize("field,other", [("fold", 0), ("c", 19), ("Wd", 14), ("fold_tile", 1 << 19), ("W", 8), ("M", 16384), ("bits", 253)])
def test_any_differing_field_splits_the_members(hset, field, other):
    a, b = dict(FOLDED), dict(FOLDED, **{field: other})
    assert classes(hset, [a, b]) == (2, [0, 1])
    assert classes(hset, [a, b, a]) == (2, [0, 1, 0])  # classes are numbered by their first member; a later equal member joins
    assert classes(hset, [b, a, a, b]) == (2, [0, 1, 1, 0])


def test_folded_beside_plain_makes_two_classes(hset):
    assert classes(hset, [FOLDED, PLAIN]) == (2, [0, 1])
    assert classes(hset, [FOLDED, PLAIN, FOLDED, PLAIN]) == (2, [0, 1, 0, 1])
    # ... even where every number but `fold` agrees
    assert classes(hset, [FOLDED, dict(FOLDED, fold=0)]) == (2, [0, 1])


def test_a_member_that_cannot_stream_is_a_class_of_its_own(hset):
    stuck = dict(FOLDED, can_train=0)
    assert classes(hset, [FOLDED, stuck, FOLDED]) == (2, [0, 1, 0])
    assert classes(hset, [stuck, stuck]) == (2, [0, 1])  # two such members never share, equal as they are
    assert classes(hset, [stuck, FOLDED, stuck, FOLDED]) == (3, [0, 1, 2, 1])


def test_class_tiles(hset, monkeypatch):
    """a class is cut as its first member's own call would be: the table's tiles for device scalars (a folded class), the
    shared-scalar pair's tiles (a plain one), the host-buffer segments when the class uploads the scalars"""
    for name in ("MLHIP_STREAM_SEGMENTS", "MLHIP_STREAM_SCHEDULE", "MLHIP_TILE_LOG2"):
        monkeypatch.delenv(name, raising=False)
    assert hset.hset_class_tiles(1, 64, 1, 0, 300) == 5
    assert hset.hset_class_tiles(1, 300, 1, 0, 300) == 1
    assert hset.hset_class_tiles(1, 1 << 20, 0, 0, (1 << 22) + 1) == 5
    assert hset.hset_class_tiles(0, 0, 1, 0, 1 << 20) == 1 and hset.hset_class_tiles(0, 0, 1, 0, 1 << 22) == 4
    assert hset.hset_class_tiles(1, 1 << 20, 1, 1, 1 << 20) == 4 and hset.hset_class_tiles(1, 1 << 20, 0, 1, 1 << 20) == 8
    assert hset.hset_class_tiles(1, 300, 1, 1, 300) == 1
    monkeypatch.setenv("MLHIP_STREAM_SEGMENTS", "5")
    assert hset.hset_class_tiles(1, 64, 1, 1, 300) == 5 and hset.hset_class_tiles(1, 64, 1, 0, 300) == 5


def test_share_switch(hset, monkeypatch):
    """MLHIP_BASES_SET_SHARE=0 / 1 decide at every size; unset, the measured thresholds do (profiles/bases_set_ab.txt): host
    scalars share from 2^12 on, device scalars from 2^16 on"""
    for dev in (0, 1):
        monkeypatch.setenv("MLHIP_BASES_SET_SHARE", "0")
        assert [hset.hset_share(n, dev) for n in (1, 300, 1 << 20)] == [0, 0, 0]
        monkeypatch.setenv("MLHIP_BASES_SET_SHARE", "1")
        assert [hset.hset_share(n, dev) for n in (1, 300, 1 << 20)] == [1, 1, 1]
        monkeypatch.delenv("MLHIP_BASES_SET_SHARE")
        least = hset.hset_share_min_n(dev)
        assert least == (1 << 16 if dev else 1 << 12)
        assert hset.hset_share(least, dev) == 1 and hset.hset_share(least - 1, dev) == 0 and hset.hset_share(1 << 22, dev) == 1
    hdr = open(os.path.join(ROOT, "mathlib_amd", "csrc", "msm_set.h")).read()
    assert re.search(r"^#define MLHIP_SET_SHARE_MIN_N_HOST \(1 << 12\)$", hdr, re.M)
    assert re.search(r"^#define MLHIP_SET_SHARE_MIN_N_DEVICE \(1 << 16\)$", hdr, re.M)
    pub = " ".join(open(os.path.join(ROOT, "include", "mlhip.h")).read().split())
    assert "2^12 host scalars / 2^16 device scalars" in pub


def test_set_create_argument_rules_without_a_device(mlhip):
    """what mlhip_bases_set_create refuses before it looks at a member: no HIP call is made, so this runs without a GPU"""
    lib = mlhip.load()
    s = ctypes.c_void_p(1)
    one = (ctypes.c_void_p * 5)()
    EINVAL = mlhip.EINVAL
    assert mlhip.mlhip_bases_set_create(lib, one, 1, None) == EINVAL
    assert mlhip.mlhip_bases_set_create(lib, one, 0, ctypes.byref(s)) == EINVAL and not s.value  # (the output is cleared first)
    assert "1 .. 4 members" in lib.mlhip_last_error().decode()
    assert mlhip.mlhip_bases_set_create(lib, one, 5, ctypes.byref(s)) == EINVAL
    assert "1 .. 4 members" in lib.mlhip_last_error().decode()
    assert mlhip.mlhip_bases_set_create(lib, None, 2, ctypes.byref(s)) == EINVAL
    assert "null member list" in lib.mlhip_last_error().decode()
    assert mlhip.mlhip_bases_set_create(lib, one, 3, ctypes.byref(s)) == EINVAL  # three null members
    assert "null member" in lib.mlhip_last_error().decode()
    info = (ctypes.c_int * 4)()
    assert mlhip.mlhip_bases_set_route(lib, None, info, 4) == EINVAL
    assert mlhip.mlhip_bases_set_route(lib, None, info, -1) == EINVAL
    with pytest.raises(mlhip.MlhipError):
        mlhip.bases_set_create(lib, [])


def test_header_inline_header_and_bindings():
    """the two names are inline functions over mlhip_bases_create / mlhip_bases_msm (include/mlhip_bases_set.h), the flags are in
    mlhip.h and in the binding, the switch is in the header's table, and the exported ABI has not grown"""
    from mathlib_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    assert re.search(r"^#define MLHIP_GROUP_SET 0x200\b", hdr, re.M) and _lib.GROUP_SET == 0x200
    assert re.search(r"^#define MLHIP_MSM_SET_ROUTE 0x100\b", hdr, re.M) and _lib.MSM_SET_ROUTE == 0x100
    assert "MLHIP_BASES_SET_SHARE=0|1" in hdr and "mlhip_bases_set.h" in hdr
    inl = open(os.path.join(ROOT, "include", "mlhip_bases_set.h")).read()
    names = ("mlhip_bases_set_create", "mlhip_bases_set_route")
    for fn in names:
        assert re.search(r"^static inline int %s\(" % fn, inl, re.M), fn
        assert callable(getattr(_lib, fn))
    fns = build.abi_functions()
    assert sorted(fns) == sorted(_lib.SYMBOLS) and not set(names) & set(fns)
    go = open(os.path.join(ROOT, "go", "driver", "hip", "hip.go")).read()
    hpp = open(os.path.join(ROOT, "include", "mlhip_driver.hpp")).read()
    for text in (go, hpp):
        assert '#include "mlhip_bases_set.h"' in text and "mlhip_bases_set_create(" in text and "mlhip_bases_set_route(" in text
    from mathlib_amd import driver

    assert callable(driver.Curve.NewBasesSet) and callable(driver.BasesSet.MultiScalarMul) and callable(driver.BasesSet.Route)
