"""Stream ordering of every entry point that takes a stream (include/mlhip.h: "in order on `stream`", "keeps no caller pointer
after return"), called the way a prover calls it: with its inputs still being produced on the stream.

The scenario (tests/stream_order_cases.py: run_scenario), for one entry point on one stream s.  Every device input starts out
holding a DECOY -- a valid input of the same shape from another seed --, the output holds 0xA5.
  1. a warm-up call on the idle stream with the real inputs (sizes every scratch buffer; first expected value)
  2. on s: the delay (k_fp_mul, calibrated to ~100 ms), then the copy of the real inputs over the decoys   -- read after write
  3. the call on s, timed on the host
  4. the host arrays it was given (offsets, base_index, q_index) are overwritten with other valid ones
  5. on s: a snapshot of the output, the decoys copied back over the inputs, the output filled with 0x5A   -- write after read
  6. `busy`: is s still working?  Asserted for every entry point that is not synchronous by contract, together with a host
     time below half the delay: the hazards were live when the call returned
  7. synchronise; the snapshot equals the warm-up, the host form on the real inputs and the CPU oracle
and three lanes of the delay's output are checked against a b^repeat in Python integers.
(a) every row of the table on a fresh stream; (b) three of them on the null stream; (c) two streams over shared scratch;
(d) the negative control: the same call on ANOTHER, idle stream sees the decoys -- the delay does hold the producer back, so an
entry point that launched on a stream other than the one it was given would fail (a).
profiles/stream_order.txt gets the calibrated delay and, per row, `busy` and the host time of the call."""
import os

import pytest

import stream_order_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

_hip_error = []


def guarded(test):
    """A failed comparison is a result; a HIP error (or any other exception) may be a fault of the device: the tests after it
    start nothing more on the GPU."""
    import functools

    @functools.wraps(test)
    def run(*args, **kwargs):
        if _hip_error:
            pytest.fail("not run: %s ended in an error that was not a comparison (%s)" % tuple(_hip_error[0]))
        try:
            return test(*args, **kwargs)
        except AssertionError:
            raise
        except BaseException as e:
            _hip_error.append((test.__name__, repr(e)[:200]))
            raise

    return run


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(scope="module")
def bench(lib, mlhip):
    """(the delay, log): the delay calibrated once and timed again -- its few small kernels must not be able to slip past it"""
    delay = S.Delay(lib, mlhip)
    lines = ["# tests/test_stream_order_gpu.py: the delay is mlhip_fp_mul_device on 2^16 lanes of BLS12-381",
             "delay: repeat %d, %.1f ms" % (delay.repeat, delay.ms),
             "# entry point, row, busy after the call (1 = the stream was still working), host time of the call"]
    assert 50.0 <= delay.ms <= 2000.0, (delay.repeat, delay.ms)
    yield delay, lines.append
    if len(lines) > 3:
        with open(os.path.join(ROOT, "profiles", "stream_order.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def _set_env(monkeypatch, case):
    for name in ("MLHIP_TILE_LOG2", "MLHIP_FIXED_BASE_MIN", "MLHIP_FB_WINDOW", "MLHIP_FB_CACHE", "MLHIP_BASES_BATCH_MAX_MB",
                 "MLHIP_G2_PREPARED_GENERAL", "MLHIP_PAIRING_QUAD", "MLHIP_MSM_BATCH_CHUNK"):
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("row", S.ROWS, ids=[r.id for r in S.ROWS])
@guarded
def test_busy_stream(lib, mlhip, bench, row, monkeypatch):
    """(a) every row on a fresh side stream"""
    import torch

    delay, log = bench
    case = row.make()
    _set_env(monkeypatch, case)
    S.run_scenario(lib, mlhip, case, torch.cuda.Stream(), delay, log, row.id, row.sync)


@pytest.mark.parametrize("entry", ["mlhip_gt_mul_device", "mlhip_msm_batch_device", "mlhip_msm_launch"])
@guarded
def test_busy_null_stream(lib, mlhip, bench, entry, monkeypatch):
    """(b) the same on the null stream"""
    import torch

    delay, log = bench
    row = S.row_for(entry)
    case = row.make()
    _set_env(monkeypatch, case)
    S.run_scenario(lib, mlhip, case, torch.cuda.default_stream(), delay, log, row.id + "@null", row.sync)


def _staged(cases):
    """device inputs, outputs (0xA5) and host arrays of several calls.  Every buffer has the size of the largest call's, the
    inputs filled up with that call's (valid) data: should a broken library run one call on another call's tables, it reads and
    writes valid memory and gives wrong bytes, not a fault."""
    import torch

    def padded(c, j):
        longest = max((o.real[j] for o in cases), key=len)
        return S.to_dev(c.real[j] + longest[len(c.real[j]):])

    ins = [[padded(c, j) for j in range(len(c.real))] for c in cases]
    outs = [[torch.full((max(o.out_bytes[j] for o in cases),), 0xA5, dtype=torch.uint8, device="cuda") for j in range(len(c.out_bytes))]
            for c in cases]
    hosts = [c.host_arrays(c.host_real) for c in cases]
    want = [c.oracle(c.real, c.host_real) for c in cases]
    torch.cuda.synchronize()
    return ins, outs, hosts, want


def _two_streams(lib, mlhip, delay, cases, warm, both_delayed=False):
    """s1 busy: the delay, then call A; s2 idle: call B at once; then call C on s1.  `warm`: the index of the call that sizes the
    shared scratch (run first, on an idle stream).
    both_delayed: s2 is busy too, with a delay of the same length queued right after the first, so that A and B become ready
    within microseconds of each other: unchained they would run side by side in the one scratch buffer.  A and B then have the same
    shape, so that even a mixture of their tables addresses valid memory."""
    import torch

    a, b, c = cases
    ins, outs, hosts, want = _staged(cases)
    s1 = torch.cuda.Stream()
    s2 = delay.independent_stream(s1)  # (two streams on one hardware queue would run one after the other whatever the library does)
    delay.clear()
    cases[warm].call(lib, mlhip, S._ptrs(ins[warm]), S._ptrs(outs[warm]), hosts[warm], s2.cuda_stream)
    torch.cuda.synchronize()
    assert [S.to_host(t)[:sz] for t, sz in zip(outs[warm], cases[warm].out_bytes)] == want[warm]
    for t in outs[warm]:
        t.fill_(0xA5)
    torch.cuda.synchronize()
    delay.queue(s1)
    if both_delayed:
        delay.queue(s2, second=True)
    a.call(lib, mlhip, S._ptrs(ins[0]), S._ptrs(outs[0]), hosts[0], s1.cuda_stream)
    b.call(lib, mlhip, S._ptrs(ins[1]), S._ptrs(outs[1]), hosts[1], s2.cuda_stream)
    c.call(lib, mlhip, S._ptrs(ins[2]), S._ptrs(outs[2]), hosts[2], s1.cuda_stream)
    busy = not s1.query()
    s1.synchronize()
    s2.synchronize()
    delay.check()
    if both_delayed:
        delay.check(second=True)
    assert busy, "the three calls returned only after the first stream had drained"
    got = [[S.to_host(t)[:sz] for t, sz in zip(o, k.out_bytes)] for o, k in zip(outs, cases)]
    assert got[0] == want[0], "call A (busy stream)"
    assert got[1] == want[1], "call B (idle stream, issued while A was waiting)"
    assert got[2] == want[2], "call C (after B, on A's stream)"


@pytest.mark.parametrize("group", [1, 2])
@guarded
def test_two_streams_msm_batch(lib, mlhip, bench, group, monkeypatch):
    """(c) the per-device scratch of the batch calls, chained through one event: B has more chunks than A and C; the warm-up is B's,
    so nothing is regrown (the regrowth's hipFree would serialise everything and hide the event chain)"""
    delay, _ = bench
    cid = group  # BLS12-381 for G1, BLS12-377 for G2
    cases = [S.MsmBatch(cid, group, 64, 1), S.MsmBatch(cid, group, 96, 2), S.MsmBatch(cid, group, 64, 3)]
    _set_env(monkeypatch, cases[0])
    _two_streams(lib, mlhip, delay, cases, 1)
    # both streams behind a delay: A and B (same K, same number of pairs, another segmentation and other inputs) become ready together
    # and C has A's shape: whatever order a broken library ran them in, every table entry addresses valid memory
    cases = [S.MsmBatch(cid, group, 64, 1), S.MsmBatch(cid, group, 64, 1, reverse=True, inputs=4), S.MsmBatch(cid, group, 64, 1, inputs=3)]
    assert len({len(c.real[0]) for c in cases}) == 1
    _two_streams(lib, mlhip, delay, cases, 0, both_delayed=True)


@pytest.mark.parametrize("group", [1, 2])
@guarded
def test_two_streams_fixed_base(lib, mlhip, bench, group, monkeypatch):
    """(c) the per-device fixed-base table: A multiplies base P on the busy stream, B base Q on the idle one, C base P again"""
    delay, _ = bench
    cid = 2 - group  # BLS12-381 for G1, BN254 for G2
    cases = [S.ScalarMul(cid, group, 0, 2048, 0), S.ScalarMul(cid, group, 0, 2048, 5), S.ScalarMul(cid, group, 0, 2048, 0)]
    assert cases[0].real[0] == cases[2].real[0] != cases[1].real[0]
    _set_env(monkeypatch, cases[0])
    _two_streams(lib, mlhip, delay, cases, 0)
    _two_streams(lib, mlhip, delay, cases, 0, both_delayed=True)  # A and B become ready together


@guarded
def test_two_streams_two_msm_plans(lib, mlhip, bench, monkeypatch):
    """(c) two plans with mlhip_msm_launch: A tiled behind the delay on s1, B tiled on the idle s2; both finished"""
    import torch

    delay, _ = bench
    a, b = S.Msm(0, 1, "launch", 10, seed=0), S.Msm(0, 1, "launch", 10, seed=7)
    _set_env(monkeypatch, a)
    ins, _, _, want = _staged([a, b])
    s1 = torch.cuda.Stream()
    s2 = delay.independent_stream(s1)
    try:
        a.open(lib, mlhip)
        b.open(lib, mlhip)
        for case, i, s in ((a, ins[0], s1), (b, ins[1], s2)):  # warm-up
            case.call(lib, mlhip, S._ptrs(i), [], {}, s.cuda_stream)
            assert case.finish(lib, mlhip) == case.oracle(case.real, {})
        delay.clear()
        delay.queue(s1)
        a.call(lib, mlhip, S._ptrs(ins[0]), [], {}, s1.cuda_stream)
        b.call(lib, mlhip, S._ptrs(ins[1]), [], {}, s2.cuda_stream)
        busy = not s1.query()
        got_b = b.finish(lib, mlhip)
        got_a = a.finish(lib, mlhip)
        torch.cuda.synchronize()
        delay.check()
        assert busy
        assert got_a == want[0] and got_b == want[1]
    finally:
        torch.cuda.synchronize()
        a.close(lib)
        b.close(lib)


@pytest.mark.parametrize("entry", ["mlhip_gt_mul_device", "mlhip_msm_batch_device"])
@guarded
def test_negative_control(lib, mlhip, bench, entry, monkeypatch):
    """(d) with the delay and the copies of the real inputs queued on s, the call on a second, idle stream gives the oracle's value
    for the DECOYS and not the one for the real inputs"""
    delay, log = bench
    row = S.row_for(entry)
    case = row.make()
    _set_env(monkeypatch, case)
    S.run_negative_control(lib, mlhip, case, delay, log, row.id)
