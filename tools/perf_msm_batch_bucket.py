#!/usr/bin/env python3
"""A/B of the bucket route of mlhip_msm_batch* (mathlib_amd/csrc/msm_batch_bucket.h) on one GPU, in one process: the device
form between events, the route off (MLHIP_MSM_BATCH_BUCKET_MIN=0) against the route forced (=9: every segment of the grid is
long), interleaved in rotating order, medians after a warm-up, every output compared byte for byte.

  grid     segment length m in {64 .. 65536} x total pairs in {2^16, 2^18, 2^20} (K = total / m segments), G1 of the three
           curves, uniform 256-bit scalars, the plan's own slice length
  slices   MLHIP_MSM_BATCH_BUCKET_SLICE swept at a few (total, m) cells
  singles  K separate mlhip_msm_g1 host-buffer calls against one mlhip_msm_batch host-buffer call (route forced), m >= 4096:
           where the Go shim's MaxBatchSegment belongs
  parent   --parent-lib PATH: this build with the route off against another build of the library (the parent commit's) on
           three all-short cells, to show that the Straus path has not moved

The default of MLHIP_MSM_BATCH_BUCKET_MIN is the smallest grid m from which the forced route is more than 4 % ahead at that
and every larger m, on all three curves, at the totals >= 2^18 (0 = never when there is none); the tool prints it.
Every step runs under a time limit: a step that passes it ends the run.

Usage: perf_msm_batch_bucket.py [--out FILE] [--parent-lib PATH] [--reps N] [--step-limit SECONDS] [--curves A,B]"""
import argparse
import ctypes
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_golden  # noqa: E402
from mathlib_amd import _lib  # noqa: E402
from mathlib_amd.build import source_hash  # noqa: E402

M_GRID = (64, 128, 256, 512, 1024, 4096, 16384, 65536)
TOTALS = (1 << 16, 1 << 18, 1 << 20)
SLICE_CELLS = ((1 << 18, 1024), (1 << 18, 16384), (1 << 20, 65536))
SLICE_SWEEP = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
SHORT_CELLS = ((1 << 16, 4), (1 << 14, 16), (1 << 10, 64))  # (segments, pairs per segment)
MARGIN = 0.04  # the pool's box-to-box spread

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_batch_bucket_ab.txt"))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-limit", type=int, default=60)
ap.add_argument("--curves", default="BN254,BLS12-381,BLS12-377")
args = ap.parse_args()

lib = _lib.load()
assert _lib.device_count() >= 1, "no GPU: nothing to measure"
parent = _lib._bind(ctypes.CDLL(args.parent_lib)) if args.parent_lib else None
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
st = stream.cuda_stream
gen = torch.Generator(device=dev)
gen.manual_seed(20)
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def step_limit(signum, frame):
    raise SystemExit("a step passed its time limit of %d s: the run ends here" % args.step_limit)


signal.signal(signal.SIGALRM, step_limit)


def rnd_scalars(k):
    return torch.randint(-(1 << 63), (1 << 63) - 1, (k, 4), dtype=torch.int64, generator=gen, device=dev).view(torch.uint8).reshape(-1).contiguous()


def set_route(t, s=None):
    os.environ["MLHIP_MSM_BATCH_BUCKET_MIN"] = str(t)
    if s is None:
        os.environ.pop("MLHIP_MSM_BATCH_BUCKET_SLICE", None)
    else:
        os.environ["MLHIP_MSM_BATCH_BUCKET_SLICE"] = str(s)


class Side:
    def __init__(self, label, library, t, s=None):
        self.label, self.library, self.t, self.s = label, library, t, s
        self.ms, self.out = [], None


def run_cell(cid, g1b, P, S, K, m, sides, reps):
    """median milliseconds of every side over reps interleaved rounds in rotating order (one warm-up round before), and
    whether all outputs are equal"""
    signal.alarm(args.step_limit)
    offs = _lib.batch_offsets([m] * K)
    n = K * m
    for sd in sides:
        sd.ms, sd.out = [], torch.zeros(K * g1b, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        for i in range(len(sides)):
            sd = sides[(i + r) % len(sides)]
            set_route(sd.t, sd.s)
            e0.record(stream)
            rc = sd.library.mlhip_msm_batch_device(cid, 1, P.data_ptr(), S.data_ptr(), 0, offs, K, sd.out.data_ptr(), st)
            e1.record(stream)
            assert rc == 0, (rc, sd.label)
            e1.synchronize()
            if r:
                sd.ms.append(e0.elapsed_time(e1))
    same = all(torch.equal(sides[0].out, sd.out) for sd in sides[1:])
    signal.alarm(0)
    assert n <= P.numel() // g1b
    return [statistics.median(sd.ms) for sd in sides], same


emit("# bucket route of mlhip_msm_batch_device against the Straus chunks: tools/perf_msm_batch_bucket.py")
emit("# source %s, device %s, %d timed rounds per cell after one warm-up, medians, device form between events" %
     (source_hash(), torch.cuda.get_device_name(0), args.reps))
ahead = {}  # (curve, total, m) -> forced is more than MARGIN ahead
all_same = True
for name in args.curves.split(","):
    g = load_golden(name)
    cid = g["curve_id"]
    _, g1b, _, _ = _lib.sizes(cid)
    nmax = max(TOTALS)
    # 4096 distinct points [s_i] G, repeated: the cost of a pair does not depend on the point
    base = torch.frombuffer(bytearray(bytes.fromhex(g["g1_gen"])), dtype=torch.uint8).to(dev)
    signal.alarm(args.step_limit)
    distinct = torch.empty(4096 * g1b, dtype=torch.uint8, device=dev)
    _lib.check(lib.mlhip_scalar_mul_device(cid, 1, base.data_ptr(), 0, rnd_scalars(4096).data_ptr(), 0, 4096, distinct.data_ptr(), st))
    P = distinct.repeat(nmax // 4096).contiguous()
    S = rnd_scalars(nmax)
    torch.cuda.synchronize()
    signal.alarm(0)
    emit()
    emit("## %s G1: route off / forced, ms (pairs per second of the faster side)" % name)
    emit("%8s %8s %8s %10s %10s %8s %6s" % ("total", "m", "K", "off ms", "forced ms", "off/frc", "equal"))
    for total in TOTALS:
        for m in M_GRID:
            if m > total:
                continue
            K = total // m
            (off, frc), same = run_cell(cid, g1b, P, S, K, m, [Side("off", lib, 0), Side("forced", lib, 9)], args.reps)
            all_same &= same
            ahead[name, total, m] = frc * (1 + MARGIN) < off
            emit("%8d %8d %8d %10.3f %10.3f %8.3f %6s   %.3g pairs/s" % (total, m, K, off, frc, off / frc, same, total / min(off, frc) * 1e3))
    emit()
    emit("## %s G1: slice length swept, route forced, ms" % name)
    emit("%8s %8s " % ("total", "m") + " ".join("%8d" % s for s in SLICE_SWEEP) + "     plan")
    for total, m in SLICE_CELLS:
        K = total // m
        sides = [Side("S=%d" % s, lib, 9, s) for s in SLICE_SWEEP] + [Side("plan", lib, 9)]
        ms, same = run_cell(cid, g1b, P, S, K, m, sides, max(3, args.reps - 2))
        all_same &= same
        emit("%8d %8d " % (total, m) + " ".join("%8.3f" % x for x in ms) + "   equal=%s" % same)
    emit()
    emit("## %s G1: K single mlhip_msm_g1 calls against one mlhip_msm_batch call (host buffers, wall clock, route forced), ms" % name)
    emit("%8s %8s %8s %12s %12s %12s" % ("total", "m", "K", "singles ms", "batch ms", "per single"))
    hp, hs = P.cpu().numpy().tobytes(), S.cpu().numpy().tobytes()
    for total in (1 << 18, 1 << 20):
        for m in (4096, 16384, 65536):
            K = total // m
            signal.alarm(args.step_limit)
            offs = _lib.batch_offsets([m] * K)
            out_b = ctypes.create_string_buffer(K * g1b)
            out_s = ctypes.create_string_buffer(K * g1b)
            set_route(9)
            tb, ts = [], []
            for r in range(3):
                t0 = time.perf_counter()
                _lib.check(lib.mlhip_msm_batch(cid, 1, hp, hs, 0, offs, K, out_b))
                tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for i in range(K):
                    o = ctypes.byref(out_s, i * g1b)
                    _lib.check(lib.mlhip_msm_g1(cid, hp[i * m * g1b : (i + 1) * m * g1b], hs[32 * i * m : 32 * (i + 1) * m], 0, m, 0, o))
                ts.append(time.perf_counter() - t0)
            signal.alarm(0)
            same = out_b.raw == out_s.raw
            all_same &= same
            emit("%8d %8d %8d %12.3f %12.3f %12.3f   equal=%s" % (total, m, K, min(ts[1:]) * 1e3, min(tb[1:]) * 1e3, min(ts[1:]) * 1e3 / K, same))
    if parent is not None:
        emit()
        emit("## %s G1: all-short batches, this build with the route off against the parent build, ms" % name)
        emit("%8s %8s %10s %10s %8s %6s" % ("K", "m", "this ms", "parent ms", "ratio", "equal"))
        for K, m in SHORT_CELLS:
            (a, b), same = run_cell(cid, g1b, P, S, K, m, [Side("this", lib, 0), Side("parent", parent, 0)], 2 * args.reps)
            all_same &= same
            emit("%8d %8d %10.3f %10.3f %8.3f %6s   %s" % (K, m, a, b, a / b, same, "within 4 %" if abs(a / b - 1) <= MARGIN else "OUTSIDE 4 %"))
    del P, S

emit()
names = args.curves.split(",")
default = 0
for m in reversed(M_GRID):
    if all(ahead.get((nm, total, m), True) for nm in names for total in TOTALS if total >= 1 << 18 and m <= total):
        default = m
    else:
        break
emit("# every output equal across sides: %s" % all_same)
emit("# rule: smallest m with the forced route more than %d %% ahead at it and every larger m, all curves, totals >= 2^18" % round(MARGIN * 100))
emit("# default MLHIP_MSM_BATCH_BUCKET_MIN by that rule: %d" % default)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
os.environ.pop("MLHIP_MSM_BATCH_BUCKET_MIN", None)
os.environ.pop("MLHIP_MSM_BATCH_BUCKET_SLICE", None)
sys.exit(0 if all_same else 1)
