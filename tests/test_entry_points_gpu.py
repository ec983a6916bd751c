"""The entry points the rest of the suite reaches only through wrappers, called by name: the device forms of the pairing and
the wire codec on a non-default stream (same bytes as the host forms, and the oracle's), the pipelined MSM pair
mlhip_msm_launch / mlhip_msm_finish two deep over two plans on two streams (as bench.py --pipelined and a Groth16 prover
drive them), the un-normalised out_xyzz sum, the plan's profiling and timings, and mlhip_sizes."""
import ctypes
import math

import numpy as np
import pytest

from wire_cases import g1_bad_encodings, g1_off_curve_uncompressed, g2_bad_encodings

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def _dev(data):
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.current_stream().synchronize()  # the tests read it on other streams
    return t


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize("curve", list(CURVES))
def test_sizes_by_name(lib, mlhip, curve):
    cid = CURVES[curve]
    a, b, c, d = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.mlhip_sizes(cid, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    fpb = 32 if cid == 0 else 48
    assert (a.value, b.value, c.value, d.value) == (fpb, 2 * fpb, 4 * fpb, 12 * fpb)
    assert lib.mlhip_sizes(7, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == mlhip.EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# pairing device forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", list(CURVES))
def test_pairing_device_forms_on_a_stream(lib, mlhip, curve, monkeypatch):
    """mlhip_miller_loop_device (ppp 1 and 4) and mlhip_final_exp_device on a non-default stream: the host forms' bytes and
    the oracle's after the final exponentiation; a planted infinity in slot 3"""
    import torch

    from oracle import cref

    for name in ("MLHIP_PAIRING_QUAD", "MLHIP_PAIRING_SAT", "MLHIP_PAIRING_ONE_LANE"):
        monkeypatch.delenv(name, raising=False)
    cid = CURVES[curve]
    _, g1b, g2b, gtb = mlhip.sizes(cid)
    n = 37  # products
    p1 = bytearray(cref.gen_points(cid, 1, 31337, 101, 4 * n))
    p2 = bytearray(cref.gen_points(cid, 2, 27182, 103, 4 * n))
    p1[3 * g1b : 4 * g1b] = bytes(g1b)  # slot 3 of product 0
    p2[9 * g2b : 10 * g2b] = bytes(g2b)
    p1, p2 = bytes(p1), bytes(p2)
    d1, d2 = _dev(p1), _dev(p2)
    s = torch.cuda.Stream()
    for ppp in (1, 4):
        raw_h = ctypes.create_string_buffer(gtb * n)
        mlhip.check(lib.mlhip_miller_loop(cid, p1, p2, ppp, n, raw_h))
        fe_h = ctypes.create_string_buffer(gtb * n)
        mlhip.check(lib.mlhip_final_exp(cid, raw_h.raw, n, fe_h))
        with torch.cuda.stream(s):
            raw_d = torch.empty(gtb * n, dtype=torch.uint8, device="cuda")
            fe_d = torch.empty_like(raw_d)
        mlhip.check(lib.mlhip_miller_loop_device(cid, d1.data_ptr(), d2.data_ptr(), ppp, n, raw_d.data_ptr(), s.cuda_stream))
        mlhip.check(lib.mlhip_final_exp_device(cid, raw_d.data_ptr(), n, fe_d.data_ptr(), s.cuda_stream))
        s.synchronize()
        assert _host(raw_d) == raw_h.raw, ppp
        assert _host(fe_d) == fe_h.raw, ppp
        want = cref.final_exp(cid, cref.miller_loop(cid, p1, p2, ppp, n, 8), n, 8)
        assert fe_h.raw == want, ppp
    assert lib.mlhip_miller_loop_device(cid, d1.data_ptr(), d2.data_ptr(), 5, 1, d1.data_ptr(), s.cuda_stream) == mlhip.EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# wire codec device forms
# ---------------------------------------------------------------------------------------------------------------------
def _codec_device(lib, mlhip, group, cid, wire, count, comp, mode, stream):
    """mlhip_g{1,2}_from_bytes_device on `stream`: (affine bytes, status bytes read back from device memory)"""
    import torch

    psz = mlhip.sizes(cid)[group]
    d_wire = _dev(wire)
    with torch.cuda.stream(stream):
        d_out = torch.full((psz * count,), 0xA5, dtype=torch.uint8, device="cuda")
        d_st = torch.full((count,), 0xEE, dtype=torch.uint8, device="cuda")
    args = (cid, d_wire.data_ptr(), count, comp, mode, d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
    if group == 1:
        mlhip.check(lib.mlhip_g1_from_bytes_device(*args))
    else:
        mlhip.check(lib.mlhip_g2_from_bytes_device(*args))
    stream.synchronize()
    return _host(d_out), _host(d_st)


def _codec_host(lib, mlhip, group, cid, wire, count, comp, mode):
    psz = mlhip.sizes(cid)[group]
    out = ctypes.create_string_buffer(psz * count)
    st = ctypes.create_string_buffer(count)
    if group == 1:
        mlhip.check(lib.mlhip_g1_from_bytes(cid, wire, count, comp, mode, out, st))
    else:
        mlhip.check(lib.mlhip_g2_from_bytes(cid, wire, count, comp, mode, out, st))
    return out.raw, st.raw


def _encode_device(lib, mlhip, group, cid, affine, count, comp, stream):
    import torch

    psz = mlhip.sizes(cid)[group]
    wlen = psz // 2 if comp else psz
    d_aff = _dev(affine)
    with torch.cuda.stream(stream):
        d_wire = torch.empty(wlen * count, dtype=torch.uint8, device="cuda")
    if group == 1:
        mlhip.check(lib.mlhip_g1_to_bytes_device(cid, d_aff.data_ptr(), count, comp, d_wire.data_ptr(), stream.cuda_stream))
    else:
        mlhip.check(lib.mlhip_g2_to_bytes_device(cid, d_aff.data_ptr(), count, comp, d_wire.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    return _host(d_wire)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", list(CURVES))
def test_wire_codec_device_forms(lib, mlhip, curve, group):
    """good points (compressed and not) and the invalid-encoding batches of the host codec tests, subgroup modes 0, 1 and 2,
    through the device forms on a non-default stream: the host forms' bytes and statuses, and pyref's statuses"""
    import torch

    from oracle import pyref as R

    cp = R.CURVES[curve]
    cid = cp.curve_id
    s = torch.cuda.Stream()
    d = R.Drbg("gpu/codec-device/%d/%s" % (group, curve))
    if group == 1:
        pts = [R.random_g1(cp, d) for _ in range(20)] + [None, cp.g1, R.g1_neg(cp, cp.g1)]
        encs = ((1, R.g1_wire_compressed), (0, R.g1_wire_uncompressed))
        to_mont, from_wire = R.g1_to_mont_bytes, R.g1_from_wire
        bad = g1_bad_encodings(R, cp, pts[0])
    else:
        g2 = R.g2_generator(cp)
        pts = [R.random_g2(cp, d) for _ in range(8)] + [None, g2, R.g2_neg(cp, g2)]
        encs = ((1, R.g2_wire_compressed), (0, R.g2_wire_uncompressed))
        to_mont, from_wire = R.g2_to_mont_bytes, R.g2_from_wire
        bad, _ = g2_bad_encodings(R, cp, pts[0])
    affine = b"".join(to_mont(cp, p) for p in pts)
    for comp, enc in encs:
        wire = b"".join(enc(cp, p) for p in pts)
        for mode in (0, 1, 2):
            out, st = _codec_device(lib, mlhip, group, cid, wire, len(pts), comp, mode, s)
            assert st == bytes(len(pts)), (comp, mode)
            assert out == affine, (comp, mode)
        assert _encode_device(lib, mlhip, group, cid, affine, len(pts), comp, s) == wire, comp
    wire = b"".join(bad)
    for mode in (0, 1, 2):
        out, st = _codec_device(lib, mlhip, group, cid, wire, len(bad), 1, mode, s)
        h_out, h_st = _codec_host(lib, mlhip, group, cid, wire, len(bad), 1, mode)
        assert st == h_st, mode
        assert list(st) == [from_wire(cp, w, mode != 0)[1] for w in bad], mode
        psz = len(affine) // len(pts)
        for i, code in enumerate(st):  # where a point decodes (status 0) its bytes are the host form's
            if code == 0:
                assert out[i * psz : (i + 1) * psz] == h_out[i * psz : (i + 1) * psz], (mode, i)
        assert out[-psz:] == to_mont(cp, pts[0]), mode
    if group == 1:
        w = g1_off_curve_uncompressed(R, cp, pts[1])
        out, st = _codec_device(lib, mlhip, 1, cid, w, 1, 0, 1, s)
        assert st == bytes([2]) == _codec_host(lib, mlhip, 1, cid, w, 1, 0, 1)[1]


# ---------------------------------------------------------------------------------------------------------------------
# the pipelined MSM: mlhip_msm_launch / mlhip_msm_finish two deep, out_xyzz, profiling
# ---------------------------------------------------------------------------------------------------------------------
def _affine_from_xyzz(cid, group, xyzz):
    """pyref: x = X / ZZ, y = Y / ZZZ (Montgomery form in and out); None for ZZ = 0"""
    from oracle import pyref as R

    cp = R.CURVES_BY_ID[cid]
    T = R.tower(cp)
    fpb = cp.fp_bytes
    k = group  # Fp elements per coordinate
    vals = [R.fp_from_mont_bytes(cp, xyzz[i * fpb : (i + 1) * fpb]) for i in range(4 * k)]
    X, Y, ZZ, ZZZ = (tuple(vals[j * k : (j + 1) * k]) for j in range(4))
    if group == 1:
        if ZZ[0] == 0:
            return None
        x = X[0] * pow(ZZ[0], -1, cp.p) % cp.p
        y = Y[0] * pow(ZZZ[0], -1, cp.p) % cp.p
        return R.g1_to_mont_bytes(cp, (x, y))
    if ZZ == (0, 0):
        return None
    x = T.f2_mul(X, T.f2_inv(ZZ))
    y = T.f2_mul(Y, T.f2_inv(ZZZ))
    return R.g2_to_mont_bytes(cp, (x, y))


def _plan(lib, mlhip, cid, group, max_n, c):
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_msm_plan_create(cid, group, max_n, c, ctypes.byref(h)))
    return h


@pytest.mark.parametrize("group", [1, 2])
def test_msm_pipelined_two_plans_two_streams(lib, mlhip, group):
    """two plans of one group on two streams, two deep: launch k + 1 on the other plan before finish k; MSMs of different n
    (0 among them, and one smaller than the previous on its plan) against cref.msm; a second launch on a pending plan is
    MLHIP_EINVAL and the pending MSM still finishes right; out_xyzz of mlhip_msm_finish and mlhip_msm_run, normalised,
    is the affine result; profiling on: 11 timing values"""
    import torch

    from oracle import cref

    cid = 1  # BLS12-381
    psz = mlhip.sizes(cid)[group]
    c = 10 if group == 1 else 8  # explicit windows: timings()[7] must report them
    max_n = 3000
    pts = cref.gen_points(cid, group, 1234567, 891, max_n)
    rng = np.random.default_rng(2024 + group)
    total = 9000
    sc = rng.integers(0, 1 << 64, size=(total, 4), dtype=np.uint64, endpoint=False)  # any 256-bit value (scalars_mont = 0)
    d_pts, d_sc = _dev(pts), _dev(sc.tobytes())
    plans = [_plan(lib, mlhip, cid, group, max_n, c) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for h in plans:
        assert lib.mlhip_msm_plan_set_profiling(h, 1) == 0
        assert lib.mlhip_msm_plan_assume_srs(h, 0) == 0
    # (n, scalar offset): plan 0 runs calls 0, 2, 4, ... and plan 1 calls 1, 3, 5, ...
    calls = [(1000, 0), (3000, 1000), (0, 0), (500, 4000), (2047, 4500), (1, 6547), (2999, 6000)]

    def launch(k):
        n, off = calls[k]
        mlhip.check(lib.mlhip_msm_launch(plans[k % 2], d_pts.data_ptr(), d_sc.data_ptr() + 32 * off, 0, n, streams[k % 2].cuda_stream))

    def expected(k):
        n, off = calls[k]
        return cref.msm(cid, group, pts, sc[off : off + n].copy(), n, False, 0, 8) if n else bytes(psz)

    launch(0)
    results = []
    for k in range(len(calls)):
        if k + 1 < len(calls):
            launch(k + 1)
        if k == 0:  # the plan of call 0 is still pending
            n, off = calls[2]
            rc = lib.mlhip_msm_launch(plans[0], d_pts.data_ptr(), d_sc.data_ptr(), 0, n, streams[0].cuda_stream)
            assert rc == mlhip.EINVAL
        out = ctypes.create_string_buffer(psz)
        xyzz = ctypes.create_string_buffer(2 * psz)
        mlhip.check(lib.mlhip_msm_finish(plans[k % 2], out, xyzz))
        results.append((out.raw, xyzz.raw))
        if calls[k][0]:
            buf = (ctypes.c_float * 11)()
            assert lib.mlhip_msm_plan_timings(plans[k % 2], buf, 11) == 11
            t = list(buf)
            assert all(math.isfinite(v) and v >= 0 for v in t[:5]) and t[4] > 0, (k, t)
            assert t[7] == c and t[9] == 0 and t[10] == 0, (k, t)
    for k, (aff, xyzz) in enumerate(results):
        assert aff == expected(k), (k, calls[k])
        norm = _affine_from_xyzz(cid, group, xyzz)
        assert (norm if norm is not None else bytes(psz)) == aff, k
    # mlhip_msm_run on the same MSM: the same affine point, and an out_xyzz that normalises to it (the projective
    # representation is not canonical: two runs of one MSM on one plan give different (X, Y, ZZ, ZZZ) bytes, include/mlhip.h)
    n, off = calls[4]
    out = ctypes.create_string_buffer(psz)
    xyzz = ctypes.create_string_buffer(2 * psz)
    mlhip.check(lib.mlhip_msm_run(plans[4 % 2], d_pts.data_ptr(), d_sc.data_ptr() + 32 * off, 0, n, streams[0].cuda_stream, out, xyzz))
    assert out.raw == results[4][0] and _affine_from_xyzz(cid, group, xyzz.raw) == out.raw
    assert lib.mlhip_msm_finish(plans[0], out, None) == mlhip.EINVAL  # nothing pending
    for h in plans:
        assert lib.mlhip_msm_plan_destroy(h) == 0


# ---------------------------------------------------------------------------------------------------------------------
# an unknown curve id through every entry point that takes one
# ---------------------------------------------------------------------------------------------------------------------
def _curve_entry_points():
    """the exported functions whose first parameter is `int curve`, from include/mlhip.h (as tests/test_api_coverage.py)"""
    import os
    import re

    from conftest import ROOT

    with open(os.path.join(ROOT, "include", "mlhip.h")) as f:
        text = f.read()
    return sorted(re.findall(r"^MLHIP_API\b[^(;]*?\b(mlhip_\w+)\s*\(\s*int\s+curve\b", text, flags=re.M))


# (return code, mlhip_last_error() contains "unknown curve id") of each of them for curve id 7 and n = k = ppp = 1, as the
# library answered when every entry point dispatched through its own `switch (curve)`: with n = 1 each of them reaches its
# curve check (curve_sizes, or the switch's default) before anything else can fail or return early; -1 = MLHIP_EINVAL
_UNKNOWN_CURVE = {
    "mlhip_bases_create": (-1, True),
    "mlhip_bases_create_device": (-1, True),
    "mlhip_bases_create_multi": (-1, True),
    "mlhip_final_exp": (-1, True),
    "mlhip_final_exp_device": (-1, True),
    "mlhip_fp_mul_device": (-1, True),
    "mlhip_g1_from_bytes": (-1, True),
    "mlhip_g1_from_bytes_device": (-1, True),
    "mlhip_g1_sum": (-1, True),
    "mlhip_g1_to_bytes": (-1, True),
    "mlhip_g1_to_bytes_device": (-1, True),
    "mlhip_g2_from_bytes": (-1, True),
    "mlhip_g2_from_bytes_device": (-1, True),
    "mlhip_g2_prepared_create": (-1, True),
    "mlhip_g2_prepared_create_device": (-1, True),
    "mlhip_g2_sum": (-1, True),
    "mlhip_g2_to_bytes": (-1, True),
    "mlhip_g2_to_bytes_device": (-1, True),
    "mlhip_gt_exp": (-1, True),
    "mlhip_gt_exp_device": (-1, True),
    "mlhip_gt_mul": (-1, True),
    "mlhip_gt_mul_device": (-1, True),
    "mlhip_miller_loop": (-1, True),
    "mlhip_miller_loop_device": (-1, True),
    "mlhip_msm_batch": (-1, True),
    "mlhip_msm_batch_device": (-1, True),
    "mlhip_msm_g1": (-1, True),
    "mlhip_msm_g1g2": (-1, True),
    "mlhip_msm_g2": (-1, True),
    "mlhip_msm_multi": (-1, True),
    "mlhip_msm_plan_create": (-1, True),
    "mlhip_pairing_batch": (-1, True),
    "mlhip_pairing_batch_device": (-1, True),
    "mlhip_pairing_product": (-1, True),
    "mlhip_scalar_mul": (-1, True),
    "mlhip_scalar_mul_device": (-1, True),
    "mlhip_sizes": (-1, True),
}


def test_unknown_curve_id_every_entry_point(lib, mlhip):
    """curve id 7 with n = 1 (k = 1, ppp = 1) through every exported function that takes a curve: the return code and whether
    the error text names the curve, against the table above.  Every pointer is a real zero-filled buffer larger than any
    curve's Gt value, so a check that moved cannot become a wild access; nothing is launched."""
    import torch

    bad = 7
    big = 4096  # bytes: a Gt value of the 48-byte fields is 576
    hb = [ctypes.create_string_buffer(big) for _ in range(5)]  # host buffers, zero-filled
    db = [torch.zeros(big, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    h0, h1, h2, h3, h4 = hb
    d0, d1, d2, d3 = (t.data_ptr() for t in db)
    st = torch.cuda.Stream().cuda_stream
    offs = mlhip.batch_offsets([1])
    devs = (ctypes.c_int * 1)(0)
    sizes = [ctypes.c_size_t() for _ in range(4)]
    handle = ctypes.c_void_p()
    hp = ctypes.byref(handle)
    calls = {
        "mlhip_sizes": lambda: lib.mlhip_sizes(bad, *(ctypes.byref(s) for s in sizes)),
        "mlhip_msm_g1": lambda: lib.mlhip_msm_g1(bad, h0, h1, 0, 1, 0, h2),
        "mlhip_msm_g2": lambda: lib.mlhip_msm_g2(bad, h0, h1, 0, 1, 0, h2),
        "mlhip_msm_g1g2": lambda: lib.mlhip_msm_g1g2(bad, h0, h1, h2, 0, 1, 0, h3, h4),
        "mlhip_msm_multi": lambda: lib.mlhip_msm_multi(bad, 1, devs, 1, h0, h1, 0, 1, 0, h2),
        "mlhip_msm_plan_create": lambda: lib.mlhip_msm_plan_create(bad, 1, 1, 0, hp),
        "mlhip_msm_batch": lambda: lib.mlhip_msm_batch(bad, 1, h0, h1, 0, offs, 1, h2),
        "mlhip_msm_batch_device": lambda: lib.mlhip_msm_batch_device(bad, 1, d0, d1, 0, offs, 1, d2, st),
        "mlhip_scalar_mul": lambda: lib.mlhip_scalar_mul(bad, 1, h0, 1, h1, 0, 1, h2),
        "mlhip_scalar_mul_device": lambda: lib.mlhip_scalar_mul_device(bad, 1, d0, 1, d1, 0, 1, d2, st),
        "mlhip_g1_sum": lambda: lib.mlhip_g1_sum(bad, h0, 1, h1),
        "mlhip_g2_sum": lambda: lib.mlhip_g2_sum(bad, h0, 1, h1),
        "mlhip_bases_create": lambda: lib.mlhip_bases_create(bad, 1, h0, 1, 0, hp),
        "mlhip_bases_create_device": lambda: lib.mlhip_bases_create_device(bad, 1, d0, 1, 0, hp),
        "mlhip_bases_create_multi": lambda: lib.mlhip_bases_create_multi(bad, 1, devs, 1, h0, 1, 0, hp),
        "mlhip_miller_loop": lambda: lib.mlhip_miller_loop(bad, h0, h1, 1, 1, h2),
        "mlhip_final_exp": lambda: lib.mlhip_final_exp(bad, h0, 1, h1),
        "mlhip_pairing_batch": lambda: lib.mlhip_pairing_batch(bad, h0, h1, 1, h2),
        "mlhip_pairing_product": lambda: lib.mlhip_pairing_product(bad, h0, h1, 1, h2),
        "mlhip_miller_loop_device": lambda: lib.mlhip_miller_loop_device(bad, d0, d1, 1, 1, d2, st),
        "mlhip_final_exp_device": lambda: lib.mlhip_final_exp_device(bad, d0, 1, d1, st),
        "mlhip_pairing_batch_device": lambda: lib.mlhip_pairing_batch_device(bad, d0, d1, 1, d2, st),
        "mlhip_gt_mul": lambda: lib.mlhip_gt_mul(bad, h0, h1, 1, h2),
        "mlhip_gt_mul_device": lambda: lib.mlhip_gt_mul_device(bad, d0, d1, 1, d2, st),
        "mlhip_gt_exp": lambda: lib.mlhip_gt_exp(bad, h0, h1, 0, 1, h2),
        "mlhip_gt_exp_device": lambda: lib.mlhip_gt_exp_device(bad, d0, d1, 0, 1, d2, st),
        "mlhip_fp_mul_device": lambda: lib.mlhip_fp_mul_device(bad, d0, d1, 1, 1, d2, st),
        "mlhip_g2_prepared_create": lambda: lib.mlhip_g2_prepared_create(bad, h0, 1, hp),
        "mlhip_g2_prepared_create_device": lambda: lib.mlhip_g2_prepared_create_device(bad, d0, 1, hp),
        "mlhip_g1_from_bytes": lambda: lib.mlhip_g1_from_bytes(bad, h0, 1, 1, 1, h1, h2),
        "mlhip_g2_from_bytes": lambda: lib.mlhip_g2_from_bytes(bad, h0, 1, 1, 1, h1, h2),
        "mlhip_g1_to_bytes": lambda: lib.mlhip_g1_to_bytes(bad, h0, 1, 1, h1),
        "mlhip_g2_to_bytes": lambda: lib.mlhip_g2_to_bytes(bad, h0, 1, 1, h1),
        "mlhip_g1_from_bytes_device": lambda: lib.mlhip_g1_from_bytes_device(bad, d0, 1, 1, 1, d1, d2, st),
        "mlhip_g2_from_bytes_device": lambda: lib.mlhip_g2_from_bytes_device(bad, d0, 1, 1, 1, d1, d2, st),
        "mlhip_g1_to_bytes_device": lambda: lib.mlhip_g1_to_bytes_device(bad, d0, 1, 1, d1, st),
        "mlhip_g2_to_bytes_device": lambda: lib.mlhip_g2_to_bytes_device(bad, d0, 1, 1, d1, st),
    }
    names = _curve_entry_points()
    assert len(names) >= 37 and set(names) == set(calls) == set(_UNKNOWN_CURVE), sorted(set(names) ^ set(calls))
    got = {}
    for name in names:
        assert lib.mlhip_set_device(99) == mlhip.EINVAL  # changes nothing but the thread's error text
        assert b"unknown curve id" not in lib.mlhip_last_error()
        rc = calls[name]()
        got[name] = (rc, b"unknown curve id" in lib.mlhip_last_error())
        print("%-34s rc %d  text %s" % ((name,) + got[name]))
        assert not handle.value, name  # no call made a handle
    torch.cuda.synchronize()
    assert got == _UNKNOWN_CURVE, {n: (got[n], _UNKNOWN_CURVE[n]) for n in names if got[n] != _UNKNOWN_CURVE[n]}
    assert all(bytes(b.raw) == bytes(big) for b in hb) and all(not t.any().item() for t in db)  # and nothing was written
