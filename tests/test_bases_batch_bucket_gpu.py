"""The bucket route on the table-free path of mlhip_bases_msm_batch / _device (mathlib_amd/csrc/msm_bases_batch.h over the
kernels of msm_batch_bucket.h, the point of a pair read through the call's index list): a handle of 24 bases with
MLHIP_BASES_BATCH_MAX_MB=0, segments long enough for several slices, with an index list (repeats, one base many times, a
base at infinity) and without one, the route forced (segments from 9 pairs, slices of 16) and off, host and device form --
all equal to cref.msm on the gathered points and to the tabled path of the same handle; and the device form on a busy
non-default stream."""
import ctypes
import random

import pytest

from bases_batch_cases import expected_indexed, gen_bases, positional_index
from msm_batch_bucket_cases import FORCED_MIN, FORCED_SLICE
from msm_batch_cases import CURVES, curve, point_bytes, sc

pytestmark = pytest.mark.gpu

N_BASES = 24
LENGTHS = [0, 40, 3, 17, 9, 70]
POSITIONAL_LENGTHS = [0, 24, 3, 17, 9, 20]  # without a list a segment of m pairs reads bases 0 .. m - 1


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def inputs(name: str, group: int):
    cp = curve(name)
    ps = point_bytes(cp, group)
    rnd = random.Random("bucket-bases-gpu/%s/%d" % (name, group))
    bases = bytearray(gen_bases(cp, group, N_BASES, 21))
    bases[5 * ps : 6 * ps] = bytes(ps)  # base 5: the point at infinity
    index = [rnd.randrange(N_BASES) for _ in range(sum(LENGTHS))]
    index[43:60] = [11] * 17  # the segment of 17 pairs: one base all the way
    index[4] = index[20] = index[69] = index[138] = 5
    scs = b"".join(sc(rnd.getrandbits(256)) for _ in range(sum(LENGTHS)))
    return cp, bytes(bases), index, scs


def force(monkeypatch, on: bool):
    monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_MIN", str(FORCED_MIN) if on else "0")
    monkeypatch.setenv("MLHIP_MSM_BATCH_BUCKET_SLICE", str(FORCED_SLICE))


class Handle:
    def __init__(self, lib, cp, group, bases: bytes):
        self.lib, self.ps = lib, point_bytes(cp, group)
        self.h = ctypes.c_void_p()
        assert lib.mlhip_bases_create(cp.curve_id, group, bases, len(bases) // self.ps, 0, ctypes.byref(self.h)) == 0

    def host(self, mlhip, scs, mont, lengths, index):
        lists = None
        if index is not None:
            lists, o = [], 0
            for m in lengths:
                lists.append(index[o : o + m])
                o += m
        return mlhip.bases_msm_batch(self.lib, self.h, self.ps, scs, mont, lengths, lists)

    def device(self, mlhip, scs, mont, lengths, index):
        import torch

        K = len(lengths)
        ds = torch.frombuffer(bytearray(scs), dtype=torch.uint8).cuda()
        out = torch.zeros(K * self.ps, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream()
        idx = mlhip.batch_index([index]) if index is not None else None
        mlhip.check(self.lib.mlhip_bases_msm_batch_device(self.h, ds.data_ptr(), 1 if mont else 0, idx, mlhip.batch_offsets(lengths), K,
                                                          st.cuda_stream, out.data_ptr()))
        st.synchronize()
        raw = out.cpu().numpy().tobytes()
        return [raw[i * self.ps : (i + 1) * self.ps] for i in range(K)]

    def close(self):
        if self.h:
            self.lib.mlhip_bases_destroy(self.h)
            self.h = ctypes.c_void_p()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", CURVES)
def test_table_free_route_forced_and_off(lib, mlhip, monkeypatch, name, group):
    cp, bases, index, scs = inputs(name, group)
    short_scs = scs[: 32 * sum(POSITIONAL_LENGTHS)]
    h = Handle(lib, cp, group, bases)
    try:
        for lengths, idx, s in ((LENGTHS, index, scs), (POSITIONAL_LENGTHS, None, short_scs)):
            gathered = idx if idx is not None else positional_index(lengths)
            exp = expected_indexed(cp, group, bases, gathered, s, lengths, False)
            monkeypatch.setenv("MLHIP_BASES_BATCH_MAX_MB", "0")
            got = {}
            for on in (True, False):
                force(monkeypatch, on)
                got[on, "host"] = h.host(mlhip, s, False, lengths, idx)
                got[on, "device"] = h.device(mlhip, s, False, lengths, idx)
            assert mlhip.bases_batch_tabled(lib, h.h) == 0  # the table-free path ran and built nothing
            for key, g in got.items():
                assert g == exp, (name, group, idx is not None, key, [i for i in range(len(g)) if g[i] != exp[i]])
        # the tabled path of the same handle, whatever the bucket switches say
        monkeypatch.delenv("MLHIP_BASES_BATCH_MAX_MB")
        force(monkeypatch, True)
        assert h.host(mlhip, scs, False, LENGTHS, index) == expected_indexed(cp, group, bases, index, scs, LENGTHS, False)
        assert mlhip.bases_batch_tabled(lib, h.h) == max(index) + 1
        # Montgomery scalars through the route
        monkeypatch.setenv("MLHIP_BASES_BATCH_MAX_MB", "0")
        assert h.host(mlhip, scs, True, LENGTHS, index) == expected_indexed(cp, group, bases, index, scs, LENGTHS, True)
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 2])
def test_device_form_on_a_busy_non_default_stream(lib, mlhip, monkeypatch, group):
    """the scalars uploaded asynchronously on the stream just before the call and overwritten on it just after; the output
    is read after a synchronize: the call is in order on the caller's stream"""
    import torch

    monkeypatch.setenv("MLHIP_BASES_BATCH_MAX_MB", "0")
    force(monkeypatch, True)
    cp, bases, index, scs = inputs("BLS12-381", group)
    ps = point_bytes(cp, group)
    K = len(LENGTHS)
    h = Handle(lib, cp, group, bases)
    try:
        hs = torch.frombuffer(bytearray(scs), dtype=torch.uint8).pin_memory()
        s = torch.cuda.Stream()
        ds = torch.zeros(len(scs), dtype=torch.uint8, device="cuda")
        out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ds.copy_(hs, non_blocking=True)
            mlhip.check(lib.mlhip_bases_msm_batch_device(h.h, ds.data_ptr(), 0, mlhip.batch_index([index]), mlhip.batch_offsets(LENGTHS),
                                                         K, s.cuda_stream, out.data_ptr()))
            ds.fill_(0x5A)
        s.synchronize()
        raw = out.cpu().numpy().tobytes()
        assert [raw[i * ps : (i + 1) * ps] for i in range(K)] == expected_indexed(cp, group, bases, index, scs, LENGTHS, False)
    finally:
        h.close()
