"""The segmented point sums on the GPU (the batch calls with MLHIP_SCALARS_UNIT; include/mlhip_sum_batch.h): for the batch of
tests/sum_batch_cases.py on every curve and group, the flagged host form and the `_device` form give oracle.pyref's
per-segment sums, the bytes of mlhip_msm_batch with an explicit array of plain-integer ones on the same points, and those of
mlhip_g1_sum / mlhip_g2_sum per segment -- with the slice length forced to 4 and at the default, with and without
MLHIP_CURVE_SUBGROUP_POINTS.  Over a handle of 40 bases: with an index list (repeats, an index used in two segments) and
without, no batch tables before or after, and a later plain mlhip_bases_msm_batch still gives its own bytes.  The Python mirror,
and the C++ one through tests/cpp/sum_batch_test.cpp."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT, load_golden
from point_sum_cases import CURVES
from sum_batch_cases import LENGTHS, TOTAL, batch, curve, indexed_batch, offsets_of, point_bytes

pytestmark = pytest.mark.gpu

ONE = (1).to_bytes(32, "little")
SLICES = ("4", None)  # MLHIP_SUM_BATCH_SLICE: forced to 4 (129 points need a middle sum pass), and the default rule


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def c_offsets(lengths):
    o = offsets_of(lengths)
    return (ctypes.c_uint64 * len(o))(*o)


def set_slice(monkeypatch, s):
    if s is None:
        monkeypatch.delenv("MLHIP_SUM_BATCH_SLICE", raising=False)
    else:
        monkeypatch.setenv("MLHIP_SUM_BATCH_SLICE", s)


def device_form(lib, mlhip, cid, group, raw, lengths, ps):
    import torch

    d_pts = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    d_out = torch.full((ps * len(lengths),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mlhip.check(mlhip.mlhip_sum_batch_device(lib, cid, group, d_pts.data_ptr(), c_offsets(lengths), len(lengths), d_out.data_ptr(), None))
    torch.cuda.synchronize()
    return bytes(d_out.cpu().numpy().tobytes())


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_flagged_calls_match_pyref_the_plain_call_with_ones_and_the_single_sums(lib, mlhip, monkeypatch, name, group):
    cp = curve(name)
    cid, ps, k = cp.curve_id, point_bytes(cp, group), len(LENGTHS)
    raw, exp = batch(name, group)
    want = b"".join(exp)
    monkeypatch.delenv("MLHIP_MSM_BATCH_BUCKET_MIN", raising=False)
    # the parent's route: explicit plain-integer ones
    out = ctypes.create_string_buffer(ps * k)
    mlhip.check(lib.mlhip_msm_batch(cid, group, raw, ONE * TOTAL, 0, c_offsets(LENGTHS), k, out))
    assert out.raw == want, "mlhip_msm_batch with explicit ones"
    # the single sums, for three segments (9, 128 and 129 points)
    fn = lib.mlhip_g1_sum if group == 1 else lib.mlhip_g2_sum
    offs = offsets_of(LENGTHS)
    for s in (6, 8, 9):
        one = ctypes.create_string_buffer(ps)
        mlhip.check(fn(cid, raw[offs[s] * ps : offs[s + 1] * ps], LENGTHS[s], one))
        assert one.raw == exp[s], ("single sum", s)
    for S in SLICES:
        set_slice(monkeypatch, S)
        out = ctypes.create_string_buffer(ps * k)
        mlhip.check(mlhip.mlhip_sum_batch(lib, cid, group, raw, c_offsets(LENGTHS), k, out))
        assert out.raw == want, ("host form", S)
        assert device_form(lib, mlhip, cid, group, raw, LENGTHS, ps) == want, ("device form", S)
        # the subgroup promise beside the flag changes nothing (the batch holds a point outside the subgroup)
        out = ctypes.create_string_buffer(ps * k)
        mlhip.check(mlhip.mlhip_sum_batch(lib, mlhip.CURVE_SUBGROUP_POINTS(cid), group, raw, c_offsets(LENGTHS), k, out))
        assert out.raw == want, ("host form with the subgroup promise", S)
    # an all-empty batch reads no point
    out = ctypes.create_string_buffer(ps * 3)
    mlhip.check(mlhip.mlhip_sum_batch(lib, cid, group, None, c_offsets([0, 0, 0]), 3, out))
    assert out.raw == bytes(ps * 3)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_sums_over_a_handle(lib, mlhip, monkeypatch, name, group):
    import torch

    cp = curve(name)
    cid, ps = cp.curve_id, point_bytes(cp, group)
    bases, lists, exp_lists, lengths, exp_lengths = indexed_batch(name, group)
    nb = len(bases) // ps
    assert nb == 40
    flat = [i for ix in lists for i in ix]
    idx = (ctypes.c_uint32 * len(flat))(*flat)
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_bases_create(cid, group, bases, nb, 0, ctypes.byref(h)))
    try:
        assert mlhip.bases_batch_tabled(lib, h) == 0
        for S in SLICES:
            set_slice(monkeypatch, S)
            k = len(lists)
            out = ctypes.create_string_buffer(ps * k)
            mlhip.check(mlhip.mlhip_bases_sum_batch(lib, h, idx, c_offsets([len(ix) for ix in lists]), k, out))
            assert out.raw == b"".join(exp_lists), ("index list", S)
            d_out = torch.full((ps * k,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            mlhip.check(mlhip.mlhip_bases_sum_batch_device(lib, h, idx, c_offsets([len(ix) for ix in lists]), k, None, d_out.data_ptr()))
            torch.cuda.synchronize()
            assert bytes(d_out.cpu().numpy().tobytes()) == b"".join(exp_lists), ("index list, device form", S)
            k = len(lengths)
            out = ctypes.create_string_buffer(ps * k)
            mlhip.check(mlhip.mlhip_bases_sum_batch(lib, h, None, c_offsets(lengths), k, out))
            assert out.raw == b"".join(exp_lengths), ("no index list", S)
            assert mlhip.bases_batch_tabled(lib, h) == 0
        # the plain call's rules that need the handle's size
        out = ctypes.create_string_buffer(ps)
        bad = (ctypes.c_uint32 * 1)(nb)
        assert mlhip.mlhip_bases_sum_batch(lib, h, bad, c_offsets([1]), 1, out) == mlhip.EINVAL
        assert b"base index out of range" in lib.mlhip_last_error()
        assert mlhip.mlhip_bases_sum_batch(lib, h, None, c_offsets([nb + 1]), 1, out) == mlhip.EINVAL
        assert b"longer than the handle's bases" in lib.mlhip_last_error()
        assert lib.mlhip_bases_msm_batch(h, ONE, mlhip.SCALARS_UNIT, None, c_offsets([1]), 1, out) == mlhip.EINVAL
        assert b"unit scalars take no scalar array" in lib.mlhip_last_error()
        s = mlhip.bases_set_create(lib, [h])
        try:
            assert mlhip.mlhip_bases_sum_batch(lib, s, None, c_offsets([1]), 1, out) == mlhip.EINVAL
            assert b"set of handles" in lib.mlhip_last_error()
        finally:
            lib.mlhip_bases_destroy(s)
        assert out.raw == bytes(ps)
        # a later plain batch on the same handle builds its tables and gives its own bytes: those of the variable-base call
        # on the gathered points with the same scalars
        import numpy as np

        sc = np.random.default_rng(5).integers(0, 1 << 64, size=(len(flat), 4), dtype=np.uint64, endpoint=False).tobytes()
        k = len(lists)
        offs = c_offsets([len(ix) for ix in lists])
        got = ctypes.create_string_buffer(ps * k)
        monkeypatch.setenv("MLHIP_BASES_BATCH_WINDOW", "6")  # narrow tables: built in a moment
        mlhip.check(lib.mlhip_bases_msm_batch(h, sc, 0, idx, offs, k, got))
        gathered = b"".join(bases[i * ps : (i + 1) * ps] for i in flat)
        ref = ctypes.create_string_buffer(ps * k)
        mlhip.check(lib.mlhip_msm_batch(cid, group, gathered, sc, 0, offs, k, ref))
        assert got.raw == ref.raw
        tabled = mlhip.bases_batch_tabled(lib, h)
        assert tabled == 40
        # ... and a flagged call after that is unchanged and leaves the tables as they are
        out = ctypes.create_string_buffer(ps * k)
        mlhip.check(mlhip.mlhip_bases_sum_batch(lib, h, idx, offs, k, out))
        assert out.raw == b"".join(exp_lists) and mlhip.bases_batch_tabled(lib, h) == tabled
    finally:
        lib.mlhip_bases_destroy(h)


def test_python_mirror(lib, mlhip):
    from mathlib_amd.driver import G1, G2, Curve

    for name, group in (("BLS12-381", 1), ("BN254", 2)):
        cp = curve(name)
        ps = point_bytes(cp, group)
        cv = Curve(cp.curve_id)
        el = G1 if group == 1 else G2
        raw, exp = batch(name, group)
        offs = offsets_of(LENGTHS)
        lists = [[el(raw[i * ps : (i + 1) * ps], cv) for i in range(a, b)] for a, b in zip(offs, offs[1:])]
        got = (cv.SumG1Batch if group == 1 else cv.SumG2Batch)(lists)
        assert [g.raw for g in got] == list(exp)
        assert got[0].IsInfinity() and (cv.SumG1Batch if group == 1 else cv.SumG2Batch)([]) == []
        bases, ilists, exp_lists, lengths, exp_lengths = indexed_batch(name, group)
        pts = [el(bases[i * ps : (i + 1) * ps], cv) for i in range(len(bases) // ps)]
        b = cv.NewBases(pts) if group == 1 else cv.NewBasesG2(pts)
        try:
            assert [g.raw for g in b.SumBatch(index_lists=ilists)] == list(exp_lists)
            assert [g.raw for g in b.SumBatch(lengths=lengths)] == list(exp_lengths)
            assert b.BatchTabled() == 0
            with pytest.raises(IndexError):
                b.SumBatch(index_lists=[[len(pts)]])
            with pytest.raises(IndexError):
                b.SumBatch(lengths=[len(pts) + 1])
            with pytest.raises(ValueError):
                b.SumBatch()
        finally:
            b.Close()


BIN = os.path.join(ROOT, "tests", "cpp", "sum_batch_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "sum_batch_test.cpp")
    hdrs = [os.path.join(ROOT, "include", f) for f in ("mlhip_driver.hpp", "mlhip_sum_batch.h", "mlhip.h")]
    lib = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in [src, lib] + hdrs):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", BIN,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    return BIN


def test_cpp_mirror():
    co = load_golden("BLS12-377")["g2_gen_coords"]
    out = subprocess.run([_build(), co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in ("BN254", "BLS12-381", "BLS12-377"):
        assert "%s sum_batch_g1 7/7 bases_index 3/3 bases_lengths 4/4" % name in out.stdout
        assert "%s sum_batch_g2 5/5" % name in out.stdout
