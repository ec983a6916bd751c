"""Stream ordering of the two `_device` forms of the segmented point sums (include/mlhip_sum_batch.h: mlhip_sum_batch_device,
mlhip_bases_sum_batch_device) on a busy stream, in the manner of tests/test_stream_order_gpu.py and with its scenario
(tests/stream_order_cases.py: run_scenario): the points are produced by work queued in front of the call, behind a ~100 ms
delay; the points, the offsets / index host arrays and the outputs are overwritten right behind the call; the bytes are
still those of the call on an idle stream, of the host form and of the CPU oracle (oracle/cref.py: an MSM with scalars 1)."""
import ctypes

import numpy as np
import pytest

import stream_order_cases as S

pytestmark = pytest.mark.gpu

ONE = (1).to_bytes(32, "little")


class SumBatch(S.Case):
    """mlhip_sum_batch_device: K segments of 0 .. 9 points, one of 70 (18 slices of 4); the offsets are host memory"""

    def __init__(self, cid, group, k=48, seed=0):
        self.cid, self.group, self.k = cid, group, k
        self.psz = 2 * group * S.FPB[cid]
        lengths = S._segments(300 + seed, k)
        lengths[3] = 70
        other = lengths[::-1]
        assert other != lengths
        total = sum(lengths)
        self.host_real = {"offsets": (ctypes.c_uint64, S._offsets(lengths))}
        self.host_other = {"offsets": (ctypes.c_uint64, S._offsets(other))}
        self.real, self.decoy = [S._pts(cid, group, 21 + seed, total)], [S._pts(cid, group, 22 + seed, total)]
        self.out_bytes = [self.psz * k]

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(mlhip.mlhip_sum_batch_device(lib, self.cid, self.group, ins[0], host["offsets"], self.k, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz * self.k)
        mlhip.check(mlhip.mlhip_sum_batch(lib, self.cid, self.group, ins[0], host["offsets"], self.k, out))
        return [out.raw]

    def oracle(self, ins, host):
        offsets = host["offsets"][1]
        return [S._msm_segments(self.cid, self.group, ins[0], ONE * offsets[-1], offsets)]


class BasesSumBatch(S.Case):
    """mlhip_bases_sum_batch_device on a 16-base handle: offsets and base_index are host memory, there is no device input"""

    def __init__(self, cid, group, indexed, k=48, nb=16):
        self.cid, self.group, self.k, self.nb, self.indexed = cid, group, k, nb, indexed
        self.psz = 2 * group * S.FPB[cid]
        self.bases = S._pts(cid, group, 23, nb)
        lengths = S._segments(310 + cid, k)
        if indexed:
            lengths[3] = 70
        total = sum(lengths)
        self.host_real = {"offsets": (ctypes.c_uint64, S._offsets(lengths))}
        self.host_other = {"offsets": (ctypes.c_uint64, S._offsets(lengths[::-1]))}
        if indexed:
            idx = [int(v) for v in np.random.default_rng(320 + cid).integers(0, nb, size=total)]
            perm = [idx[i] for i in np.random.default_rng(321).permutation(total)]
            assert perm != idx
            self.host_real["base_index"] = (ctypes.c_uint32, idx)
            self.host_other["base_index"] = (ctypes.c_uint32, perm)
        self.real, self.decoy = [], []
        self.out_bytes = [self.psz * k]
        self.h = None

    def open(self, lib, mlhip):
        self.h = ctypes.c_void_p()
        mlhip.check(lib.mlhip_bases_create(self.cid, self.group, self.bases, self.nb, 0, ctypes.byref(self.h)))

    def close(self, lib):
        if self.h:
            lib.mlhip_bases_destroy(self.h)
            self.h = None

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(mlhip.mlhip_bases_sum_batch_device(lib, self.h, host.get("base_index"), host["offsets"], self.k, stream, outs[0]))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz * self.k)
        mlhip.check(mlhip.mlhip_bases_sum_batch(lib, self.h, host.get("base_index"), host["offsets"], self.k, out))
        return [out.raw]

    def oracle(self, ins, host):
        offsets = host["offsets"][1]
        if self.indexed:
            index = host["base_index"][1]
        else:
            index = [i - a for a, b in zip(offsets, offsets[1:]) for i in range(a, b)]
        return [S._msm_segments(self.cid, self.group, self.bases, ONE * offsets[-1], offsets, index)]


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(scope="module")
def delay(lib, mlhip):
    d = S.Delay(lib, mlhip)
    assert 50.0 <= d.ms <= 2000.0, (d.repeat, d.ms)
    return d


CASES = [
    ("sum_batch:g1", lambda: SumBatch(1, 1)),
    ("sum_batch:g2", lambda: SumBatch(2, 2)),
    ("bases_sum_batch:g1,indexed", lambda: BasesSumBatch(1, 1, True)),
    ("bases_sum_batch:g2,indexed", lambda: BasesSumBatch(0, 2, True)),
    ("bases_sum_batch:g1,positional", lambda: BasesSumBatch(2, 1, False)),
]


@pytest.mark.parametrize("label,make", CASES, ids=[c[0] for c in CASES])
def test_busy_stream(lib, mlhip, delay, label, make, monkeypatch):
    import torch

    monkeypatch.setenv("MLHIP_SUM_BATCH_SLICE", "4")
    seen = []
    out = S.run_scenario(lib, mlhip, make(), torch.cuda.Stream(), delay, seen.append, label)
    assert out.busy and len(seen) == 1
