"""The Gt wire codec, the membership test and Gt.Inverse on the GPU (mathlib_amd/csrc/gt_codec.h): mlhip_gt_from_bytes /
to_bytes / is_member / inverse and their _device forms against oracle/pyref.py on every value of tests/gt_codec_cases.py --
members, values outside Gt of every kind, malformed encodings -- every curve, the quad kernels (default) and the lane-pair
kernels (MLHIP_PAIRING_QUAD=0), batch sizes that leave a partial last block in both (a 64-lane block holds 16 quads or 32
pairs; the codec kernels hold 16 values per block).  Every element's status and bytes are compared."""
import ctypes
import functools

import pytest

from gt_codec_cases import CURVES, inverse_bytes, wires

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 17, 33, 67)
IDS = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(params=["quad", "pairs"])
def family(request, monkeypatch):
    """which kernels run: read per call, as tests/test_gt_exp_cyclo_gpu.py selects them"""
    if request.param == "pairs":
        monkeypatch.setenv("MLHIP_PAIRING_QUAD", "0")
    else:
        monkeypatch.delenv("MLHIP_PAIRING_QUAD", raising=False)
    return request.param


@functools.lru_cache(maxsize=None)
def batch(name):
    """67 elements cycling the 16 cases: (wire, status with the check, in-memory value or zeros, in-memory inverse, member)"""
    from oracle import pyref as R

    cp = R.CURVES[name]
    gtb = 12 * cp.fp_bytes
    inv = inverse_bytes(name)
    rows = []
    for w in wires(name):
        if w.f is None:
            rows.append((w.wire, w.status, bytes(gtb), bytes(gtb), False, False))
        else:
            rows.append((w.wire, w.status, R.gt_to_mont_bytes(cp, w.f), inv[w.label], w.status == 0, True))
    return [rows[i % len(rows)] for i in range(max(SIZES))], {w.label: w for w in wires(name)}


def _chunks(raw, size, n):
    return [raw[i * size : (i + 1) * size] for i in range(n)]


@pytest.mark.parametrize("curve", CURVES)
def test_host_forms_against_the_oracle(lib, mlhip, curve, family):
    from oracle import pyref as R

    cid = IDS[curve]
    cp = R.CURVES[curve]
    T = R.tower(cp)
    gtb = 12 * cp.fp_bytes
    rows, _ = batch(curve)
    for n in SIZES:
        wire = b"".join(r[0] for r in rows[:n])
        cap = max(n, 1)
        out1, out0, enc, back, inv = (ctypes.create_string_buffer(gtb * cap) for _ in range(5))
        st1, st0, stm, stb = (ctypes.create_string_buffer(b"\xee" * cap, cap) for _ in range(4))
        mlhip.check(lib.mlhip_gt_from_bytes(cid, wire, n, 1, out1, st1))
        mlhip.check(lib.mlhip_gt_from_bytes(cid, wire, n, 0, out0, st0))
        mlhip.check(lib.mlhip_gt_to_bytes(cid, out0.raw[: gtb * n], n, enc))
        mlhip.check(lib.mlhip_gt_is_member(cid, out0.raw[: gtb * n], n, stm))
        mlhip.check(lib.mlhip_gt_from_bytes(cid, enc.raw[: gtb * n], n, 0, back, stb))
        mlhip.check(lib.mlhip_gt_inverse(cid, out0.raw[: gtb * n], n, inv))
        if n == 0:  # nothing written
            assert out1.raw == out0.raw == enc.raw == inv.raw == bytes(gtb) and st1.raw == st0.raw == stm.raw == b"\xee"
            continue
        tag = (curve, family, n)
        # statuses: as the case file says with the check, 0 / 1 only without; outputs all zero where the status is not 0
        assert list(st1.raw) == [r[1] for r in rows[:n]], tag
        assert list(st0.raw) == [0 if r[5] else 1 for r in rows[:n]], tag
        assert _chunks(out1.raw, gtb, n) == [r[2] if r[1] == 0 else bytes(gtb) for r in rows[:n]], tag
        assert _chunks(out0.raw, gtb, n) == [r[2] for r in rows[:n]], tag
        # to_bytes equals gt_wire_bytes (a malformed element decoded to zeros, which encode to zeros), and comes back
        assert _chunks(enc.raw, gtb, n) == [r[0] if r[5] else bytes(gtb) for r in rows[:n]], tag
        assert _chunks(back.raw, gtb, n) == [r[2] for r in rows[:n]] and stb.raw == bytes(n), tag
        # is_member agrees with from_bytes on every well-formed element (0 -- what a malformed one became -- is outside Gt)
        assert list(stm.raw) == [0 if r[4] else 3 for r in rows[:n]], tag
        assert all(stm.raw[j] == st1.raw[j] for j in range(n) if rows[j][5]), tag
        # the inverse: pyref's f12_inv on every well-formed case, 0 for 0; on members the conjugate
        assert _chunks(inv.raw, gtb, n) == [r[3] for r in rows[:n]], tag
        for j, r in enumerate(rows[:n]):
            if r[4]:
                assert inv.raw[j * gtb : (j + 1) * gtb] == R.gt_to_mont_bytes(cp, T.f12_conj(R.gt_from_mont_bytes(cp, r[2]))), tag


@pytest.mark.parametrize("curve", CURVES)
def test_device_forms_equal_the_host_forms(lib, mlhip, curve, family):
    """on a side stream, torch-allocated buffers"""
    import torch

    cid = IDS[curve]
    gtb = 12 * (32 if cid == 0 else 48)
    rows, _ = batch(curve)
    st = torch.cuda.Stream()

    def dev(raw):
        return torch.frombuffer(bytearray(raw or bytes(1)), dtype=torch.uint8).cuda()

    for n in SIZES:
        wire = b"".join(r[0] for r in rows[:n])
        vals = b"".join(r[2] for r in rows[:n])
        cap = max(n, 1)
        h_out, h_enc, h_inv = (ctypes.create_string_buffer(gtb * cap) for _ in range(3))
        h_st, h_stm = (ctypes.create_string_buffer(cap) for _ in range(2))
        d_wire, d_vals = dev(wire), dev(vals)
        d_out1, d_out0, d_enc, d_inv = (torch.zeros(gtb * cap, dtype=torch.uint8, device="cuda") for _ in range(4))
        d_st1, d_st0, d_stm = (torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        s = st.cuda_stream
        mlhip.check(lib.mlhip_gt_from_bytes_device(cid, d_wire.data_ptr(), n, 1, d_out1.data_ptr(), d_st1.data_ptr(), s))
        mlhip.check(lib.mlhip_gt_from_bytes_device(cid, d_wire.data_ptr(), n, 0, d_out0.data_ptr(), d_st0.data_ptr(), s))
        mlhip.check(lib.mlhip_gt_to_bytes_device(cid, d_vals.data_ptr(), n, d_enc.data_ptr(), s))
        mlhip.check(lib.mlhip_gt_is_member_device(cid, d_vals.data_ptr(), n, d_stm.data_ptr(), s))
        mlhip.check(lib.mlhip_gt_inverse_device(cid, d_vals.data_ptr(), n, d_inv.data_ptr(), s))
        st.synchronize()
        got = [t.cpu().numpy().tobytes() for t in (d_out1, d_st1, d_out0, d_st0, d_enc, d_stm, d_inv)]
        if n == 0:
            assert got == [bytes(gtb), b"\xee", bytes(gtb), b"\xee", bytes(gtb), b"\xee", bytes(gtb)]
            continue
        tag = (curve, family, n)
        mlhip.check(lib.mlhip_gt_from_bytes(cid, wire, n, 1, h_out, h_st))
        assert got[0] == h_out.raw and got[1] == h_st.raw, tag
        mlhip.check(lib.mlhip_gt_from_bytes(cid, wire, n, 0, h_out, h_st))
        assert got[2] == h_out.raw and got[3] == h_st.raw, tag
        mlhip.check(lib.mlhip_gt_to_bytes(cid, vals, n, h_enc))
        mlhip.check(lib.mlhip_gt_is_member(cid, vals, n, h_stm))
        mlhip.check(lib.mlhip_gt_inverse(cid, vals, n, h_inv))
        assert got[4] == h_enc.raw and got[5] == h_stm.raw and got[6] == h_inv.raw, tag
        assert list(got[5]) == [0 if r[4] else 3 for r in rows[:n]], tag


@pytest.mark.parametrize("curve", CURVES)
def test_what_passes_is_member_keeps_the_promise_of_gt_exp_cyclo(lib, mlhip, curve, family):
    """the inputs that pass mlhip_gt_is_member go through mlhip_gt_exp_cyclo and mlhip_gt_exp: byte for byte the same"""
    import numpy as np

    cid = IDS[curve]
    gtb = 12 * (32 if cid == 0 else 48)
    rows, _ = batch(curve)
    n = 33
    vals = b"".join(r[2] for r in rows[:n])
    stm = ctypes.create_string_buffer(n)
    mlhip.check(lib.mlhip_gt_is_member(cid, vals, n, stm))
    passed = [j for j in range(n) if stm.raw[j] == 0]
    assert passed == [j for j in range(n) if rows[j][4]] and len(passed) >= 10
    ins = b"".join(vals[j * gtb : (j + 1) * gtb] for j in passed)
    sc = np.random.default_rng(99 + cid).integers(0, 1 << 63, size=(len(passed), 4), dtype=np.uint64).tobytes()
    fast, slow = (ctypes.create_string_buffer(gtb * len(passed)) for _ in range(2))
    mlhip.check(lib.mlhip_gt_exp_cyclo(cid, ins, sc, 0, len(passed), fast))
    mlhip.check(lib.mlhip_gt_exp(cid, ins, sc, 0, len(passed), slow))
    assert fast.raw == slow.raw


def test_argument_errors(lib, mlhip):
    """curve id 9 and a null pointer with n > 0 through all eight entry points: MLHIP_EINVAL, zero-filled buffers larger than
    any Gt value stay zero, nothing is launched"""
    import torch

    big = 4096
    h = [ctypes.create_string_buffer(big) for _ in range(3)]
    d = [torch.zeros(big, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream().cuda_stream
    d0, d1, d2 = (t.data_ptr() for t in d)
    for cid, a, b, c, x, y, z in ((9, h[0], h[1], h[2], d0, d1, d2), (1, None, h[1], h[2], None, d1, d2), (1, h[0], None, h[2], d0, None, d2)):
        rcs = [
            lib.mlhip_gt_from_bytes(cid, a, 1, 1, b, c),
            lib.mlhip_gt_to_bytes(cid, a, 1, b),
            lib.mlhip_gt_is_member(cid, a, 1, b),
            lib.mlhip_gt_inverse(cid, a, 1, b),
            lib.mlhip_gt_from_bytes_device(cid, x, 1, 1, y, z, st),
            lib.mlhip_gt_to_bytes_device(cid, x, 1, y, st),
            lib.mlhip_gt_is_member_device(cid, x, 1, y, st),
            lib.mlhip_gt_inverse_device(cid, x, 1, y, st),
        ]
        assert rcs == [mlhip.EINVAL] * 8, (cid, rcs)
        assert (b"unknown curve id" in lib.mlhip_last_error()) == (cid == 9)
    assert lib.mlhip_gt_from_bytes(1, h[0], 1, 1, h[1], None) == mlhip.EINVAL
    assert lib.mlhip_gt_from_bytes_device(1, d0, 1, 1, d1, None, st) == mlhip.EINVAL
    torch.cuda.synchronize()
    assert all(bytes(b.raw) == bytes(big) for b in h) and all(not t.any().item() for t in d)
