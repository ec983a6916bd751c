"""The G2 bucket route of the batched MSM on the GPU (the lane-pair kernels of mathlib_amd/csrc/msm_batch_bucket.h behind
mlhip_msm_batch / mlhip_msm_batch_device): every case of tests/msm_batch_bucket_g2_cases.py with the route forced (segments
from 9 pairs, slices of 16) and with it off, both equal to cref.msm and to each other, through the host-buffer and the
device form, with Montgomery and plain scalars; each case alone; a batch at the default settings and with the plan's own
slices; one long segment against mlhip_msm_g2; the device form on a busy non-default stream."""
import ctypes
import functools

import pytest

from msm_batch_bucket_g2_cases import CURVES, FORCED_MIN, FORCED_SLICE, cases, curve
from msm_batch_cases import expected, point_bytes, random_segments

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def force(monkeypatch, on: bool):
    monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_MIN", str(FORCED_MIN) if on else "0")
    monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_SLICE", str(FORCED_SLICE))


@functools.lru_cache(maxsize=None)
def joined(name: str):
    """all cases of a curve as ONE batch (the segments of every case one after the other) and its expected bytes"""
    cp = curve(name)
    pts = b"".join(c[1] for c in cases(name))
    scs = b"".join(c[2] for c in cases(name))
    lengths = [m for c in cases(name) for m in c[3]]
    return pts, scs, lengths, {mont: expected(cp, 2, pts, scs, lengths, mont) for mont in (False, True)}


def device_form(lib, mlhip, cp, pts, scs, lengths, mont):
    import torch

    ps = point_bytes(cp, 2)
    K = len(lengths)
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    ds = torch.frombuffer(bytearray(scs), dtype=torch.uint8).cuda()
    out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    mlhip.check(lib.mlhip_msm_batch_device(cp.curve_id, 2, dp.data_ptr(), ds.data_ptr(), 1 if mont else 0,
                                           mlhip.batch_offsets(lengths), K, out.data_ptr(), st.cuda_stream))
    st.synchronize()
    raw = out.cpu().numpy().tobytes()
    return [raw[i * ps : (i + 1) * ps] for i in range(K)]


@pytest.mark.parametrize("name", CURVES)
def test_cases_forced_and_off_match_cref(lib, mlhip, monkeypatch, name):
    cp = curve(name)
    pts, scs, lengths, exp = joined(name)
    got = {}
    for mont in (False, True):
        for on in (True, False):
            force(monkeypatch, on)
            got[mont, on, "host"] = mlhip.msm_batch(cp.curve_id, 2, pts, scs, mont, lengths)
            got[mont, on, "device"] = device_form(lib, mlhip, cp, pts, scs, lengths, mont)
    assert len(got) == 8
    for key, g in got.items():
        assert g == exp[key[0]], (name, key, [i for i in range(len(g)) if g[i] != exp[key[0]][i]][:10])
    for mont in (False, True):  # (the same scalar bytes read in the other form are other scalars)
        assert got[mont, True, "host"] == got[mont, False, "host"] == got[mont, True, "device"] == got[mont, False, "device"]


@pytest.mark.parametrize("name", CURVES)
def test_each_case_alone_forced(lib, mlhip, monkeypatch, name):
    """every case as a call of its own (its slices are then the call's first rows), plain scalars"""
    cp = curve(name)
    force(monkeypatch, True)
    for case, pts, scs, lengths in cases(name):
        got = mlhip.msm_batch(cp.curve_id, 2, pts, scs, False, lengths)
        exp = expected(cp, 2, pts, scs, lengths, False)
        assert got == exp, (name, case, [i for i in range(len(exp)) if got[i] != exp[i]])


@pytest.mark.parametrize("name", CURVES)
def test_default_settings_batch(lib, mlhip, monkeypatch, name):
    monkeypatch.delenv("MLHIP_MSM_BATCH_BUCKET_MIN", raising=False)
    monkeypatch.delenv("MLHIP_MSM_BATCH_BUCKET_SLICE", raising=False)
    cp = curve(name)
    pts, scs, lengths = random_segments(cp, 2, [1500, 600, 1, 0, 64], "bucket-g2-default/" + name)
    got = mlhip.msm_batch(cp.curve_id, 2, pts, scs, False, lengths)
    assert got == expected(cp, 2, pts, scs, lengths, False)
    # the same batch with the plan's own slices from 64 pairs on, and from 9 on
    for t in (64, 9):
        monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_MIN", str(t))
        assert mlhip.msm_batch(cp.curve_id, 2, pts, scs, False, lengths) == got, t


@pytest.mark.parametrize("name", CURVES)
def test_one_long_segment_equals_msm_g2(lib, mlhip, monkeypatch, name):
    cp = curve(name)
    pts, scs, lengths = random_segments(cp, 2, [1500], "bucket-g2-single/" + name)
    out = ctypes.create_string_buffer(point_bytes(cp, 2))
    mlhip.check(lib.mlhip_msm_g2(cp.curve_id, pts, scs, 0, 1500, 0, out))
    monkeypatch.delenv("MLHIP_MSM_BATCH_BUCKET_SLICE", raising=False)
    for t in (None, 9, 0):
        if t is None:
            monkeypatch.delenv("MLHIP_MSM_BATCH_BUCKET_MIN", raising=False)
        else:
            monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_MIN", str(t))
        assert mlhip.msm_batch(cp.curve_id, 2, pts, scs, False, lengths) == [out.raw], (name, t)


def test_device_form_on_a_busy_non_default_stream(lib, mlhip, monkeypatch):
    """inputs uploaded asynchronously on the stream just before the call and overwritten on it just after; the output is
    read after a synchronize: the call is in order on the caller's stream"""
    import torch

    force(monkeypatch, True)
    cp = curve("BLS12-381")
    pts, scs, lengths, exp = joined("BLS12-381")
    ps = point_bytes(cp, 2)
    K = len(lengths)
    hp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).pin_memory()
    hs = torch.frombuffer(bytearray(scs), dtype=torch.uint8).pin_memory()
    s = torch.cuda.Stream()
    dp = torch.zeros(len(pts), dtype=torch.uint8, device="cuda")
    ds = torch.zeros(len(scs), dtype=torch.uint8, device="cuda")
    out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dp.copy_(hp, non_blocking=True)
        ds.copy_(hs, non_blocking=True)
        mlhip.check(lib.mlhip_msm_batch_device(cp.curve_id, 2, dp.data_ptr(), ds.data_ptr(), 0, mlhip.batch_offsets(lengths), K,
                                               out.data_ptr(), s.cuda_stream))
        dp.fill_(0xA5)
        ds.fill_(0x5A)
    s.synchronize()
    raw = out.cpu().numpy().tobytes()
    assert [raw[i * ps : (i + 1) * ps] for i in range(K)] == exp[False]
