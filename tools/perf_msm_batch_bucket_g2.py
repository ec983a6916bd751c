#!/usr/bin/env python3
"""A/B of the two newer uses of the bucket route (mathlib_amd/csrc/msm_batch_bucket.h) on one GPU, in one process, by the
protocol of tools/perf_msm_batch_bucket.py: the device form between events, the route off (MLHIP_MSM_BATCH_BUCKET_MIN=0)
against the route forced (=9: every segment of the grid is long), interleaved in rotating order, medians after a warm-up,
uniform 256-bit scalars, every output compared byte for byte.

  g2       mlhip_msm_batch_device, G2 of the three curves: segment length m in {64 .. 16384} x total pairs in {2^16, 2^18}
           (K = total / m segments), the plan's own slice length
  slices   MLHIP_MSM_BATCH_BUCKET_SLICE swept at two (total, m) cells of G2
  bases    mlhip_bases_msm_batch_device on its table-free path (MLHIP_BASES_BATCH_MAX_MB=0), G1, a handle of 4096 bases read
           through a random index list: the same m at 2^18 and 2^20 pairs
  parent   --parent-lib PATH: this build with the route off against another build of the library (the parent commit's) on
           G2 2^14 x 4 and 2^10 x 64 and G1 2^16 x 4, to show that the Straus path has not moved

The default of MLHIP_MSM_BATCH_BUCKET_MIN for G2 is the smallest grid m from which the forced route is more than 4 % ahead
at that and every larger m, on all three curves, at both totals (0 = never when there is none); the tool prints it, and
the same figure for the table-free G1 path.  Every step runs under a time limit: a step that passes it ends the run.

Usage: perf_msm_batch_bucket_g2.py [--out FILE] [--parent-lib PATH] [--reps N] [--step-limit SECONDS] [--curves A,B]"""
import argparse
import ctypes
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_golden  # noqa: E402
from mathlib_amd import _lib  # noqa: E402
from mathlib_amd.build import source_hash  # noqa: E402

M_GRID = (64, 128, 256, 512, 1024, 4096, 16384)
G2_TOTALS = (1 << 16, 1 << 18)
BASES_TOTALS = (1 << 18, 1 << 20)
N_BASES = 4096
SLICE_CELLS = ((1 << 18, 1024), (1 << 18, 16384))
SLICE_SWEEP = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
PARENT_CELLS = ((2, 1 << 14, 4), (2, 1 << 10, 64), (1, 1 << 16, 4))  # (group, segments, pairs per segment)
MARGIN = 0.04  # the pool's box-to-box spread

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_batch_bucket_g2_ab.txt"))
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
gen.manual_seed(21)
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


def run_cell(call, out_bytes, sides, reps):
    """median milliseconds of every side over reps interleaved rounds in rotating order (one warm-up round before), and
    whether all outputs are equal; call(side) queues the side's library call on the stream and returns its code"""
    signal.alarm(args.step_limit)
    for sd in sides:
        sd.ms, sd.out = [], torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        for i in range(len(sides)):
            sd = sides[(i + r) % len(sides)]
            set_route(sd.t, sd.s)
            e0.record(stream)
            rc = call(sd)
            e1.record(stream)
            assert rc == 0, (rc, sd.label)
            e1.synchronize()
            if r:
                sd.ms.append(e0.elapsed_time(e1))
    same = all(torch.equal(sides[0].out, sd.out) for sd in sides[1:])
    signal.alarm(0)
    return [statistics.median(sd.ms) for sd in sides], same


def batch_call(cid, group, P, S, K, m):
    offs = _lib.batch_offsets([m] * K)
    return lambda sd: sd.library.mlhip_msm_batch_device(cid, group, P.data_ptr(), S.data_ptr(), 0, offs, K, sd.out.data_ptr(), st)


def points_of(cid, group, gen_hex, size, n):
    """n points: 4096 distinct [s_i] G, repeated (the cost of a pair does not depend on the point)"""
    signal.alarm(args.step_limit)
    base = torch.frombuffer(bytearray(bytes.fromhex(gen_hex)), dtype=torch.uint8).to(dev)
    distinct = torch.empty(4096 * size, dtype=torch.uint8, device=dev)
    _lib.check(lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, rnd_scalars(4096).data_ptr(), 0, 4096, distinct.data_ptr(), st))
    P = distinct.repeat(max(1, n // 4096)).contiguous()
    torch.cuda.synchronize()
    signal.alarm(0)
    return P


def rule(ahead, names, totals):
    default = 0
    for m in reversed(M_GRID):
        if all(ahead.get((nm, total, m), True) for nm in names for total in totals if m <= total):
            default = m
        else:
            break
    return default


emit("# bucket route against the Straus chunks, G2 and the table-free path of mlhip_bases_msm_batch_device: tools/perf_msm_batch_bucket_g2.py")
emit("# source %s, device %s, %d timed rounds per cell after one warm-up, medians, device form between events" %
     (source_hash(), torch.cuda.get_device_name(0), args.reps))
ahead_g2, ahead_bases = {}, {}
all_same = True
names = args.curves.split(",")
for name in names:
    g = load_golden(name)
    cid = g["curve_id"]
    _, g1b, g2b, _ = _lib.sizes(cid)
    S = rnd_scalars(max(BASES_TOTALS))
    P2 = points_of(cid, 2, g["g2_gen"], g2b, max(G2_TOTALS))
    emit()
    emit("## %s G2: route off / forced, ms (pairs per second of the faster side)" % name)
    emit("%8s %8s %8s %10s %10s %8s %6s" % ("total", "m", "K", "off ms", "forced ms", "off/frc", "equal"))
    for total in G2_TOTALS:
        for m in M_GRID:
            K = total // m
            (off, frc), same = run_cell(batch_call(cid, 2, P2, S, K, m), K * g2b, [Side("off", lib, 0), Side("forced", lib, 9)], args.reps)
            all_same &= same
            ahead_g2[name, total, m] = frc * (1 + MARGIN) < off
            emit("%8d %8d %8d %10.3f %10.3f %8.3f %6s   %.3g pairs/s" % (total, m, K, off, frc, off / frc, same, total / min(off, frc) * 1e3))
    emit()
    emit("## %s G2: slice length swept, route forced, ms" % name)
    emit("%8s %8s " % ("total", "m") + " ".join("%8d" % s for s in SLICE_SWEEP) + "     plan")
    for total, m in SLICE_CELLS:
        K = total // m
        sides = [Side("S=%d" % s, lib, 9, s) for s in SLICE_SWEEP] + [Side("plan", lib, 9)]
        ms, same = run_cell(batch_call(cid, 2, P2, S, K, m), K * g2b, sides, max(3, args.reps - 2))
        all_same &= same
        emit("%8d %8d " % (total, m) + " ".join("%8.3f" % x for x in ms) + "   equal=%s" % same)
    # the table-free path of a G1 handle
    P1 = points_of(cid, 1, g["g1_gen"], g1b, N_BASES)
    handle = ctypes.c_void_p()
    _lib.check(lib.mlhip_bases_create(cid, 1, P1.cpu().numpy().tobytes(), N_BASES, 0, ctypes.byref(handle)))
    os.environ["MLHIP_BASES_BATCH_MAX_MB"] = "0"
    index = torch.randint(0, N_BASES, (max(BASES_TOTALS),), dtype=torch.int32, generator=gen, device=dev).cpu().numpy()
    idx = index.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    emit()
    emit("## %s G1, table-free path of mlhip_bases_msm_batch_device (%d bases, random index list): route off / forced, ms" % (name, N_BASES))
    emit("%8s %8s %8s %10s %10s %8s %6s" % ("total", "m", "K", "off ms", "forced ms", "off/frc", "equal"))
    for total in BASES_TOTALS:
        for m in M_GRID:
            K = total // m
            offs = _lib.batch_offsets([m] * K)
            call = lambda sd: sd.library.mlhip_bases_msm_batch_device(handle, S.data_ptr(), 0, idx, offs, K, st, sd.out.data_ptr())  # noqa: E731
            (off, frc), same = run_cell(call, K * g1b, [Side("off", lib, 0), Side("forced", lib, 9)], args.reps)
            all_same &= same
            ahead_bases[name, total, m] = frc * (1 + MARGIN) < off
            emit("%8d %8d %8d %10.3f %10.3f %8.3f %6s   %.3g pairs/s" % (total, m, K, off, frc, off / frc, same, total / min(off, frc) * 1e3))
    torch.cuda.synchronize()
    n_tabled = ctypes.c_size_t(1)
    _lib.check(lib.mlhip_bases_batch_tabled(handle, ctypes.byref(n_tabled)))
    assert n_tabled.value == 0, "the handle built tables: this was not the table-free path"
    _lib.check(lib.mlhip_bases_destroy(handle))
    os.environ.pop("MLHIP_BASES_BATCH_MAX_MB", None)
    if parent is not None:
        emit()
        emit("## %s: all-short batches, this build with the route off against the parent build, ms" % name)
        emit("%6s %8s %8s %10s %10s %8s %6s" % ("group", "K", "m", "this ms", "parent ms", "ratio", "equal"))
        P1n = points_of(cid, 1, g["g1_gen"], g1b, 1 << 18)
        for group, K, m in PARENT_CELLS:
            P, size = (P1n, g1b) if group == 1 else (P2, g2b)
            (a, b), same = run_cell(batch_call(cid, group, P, S, K, m), K * size, [Side("this", lib, 0), Side("parent", parent, 0)],
                                    2 * args.reps)
            all_same &= same
            emit("%6s %8d %8d %10.3f %10.3f %8.3f %6s   %s" % ("G%d" % group, K, m, a, b, a / b, same,
                                                             "within 4 %" if abs(a / b - 1) <= MARGIN else "OUTSIDE 4 %"))
        del P1n
    del P1, P2, S

emit()
emit("# every output equal across sides: %s" % all_same)
emit("# rule: smallest m with the forced route more than %d %% ahead at it and every larger m, all curves, both totals" % round(MARGIN * 100))
emit("# default MLHIP_MSM_BATCH_BUCKET_MIN for G2 by that rule: %d" % rule(ahead_g2, names, G2_TOTALS))
emit("# the same figure for the table-free G1 path (it uses G1's default): %d" % rule(ahead_bases, names, BASES_TOTALS))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
os.environ.pop("MLHIP_MSM_BATCH_BUCKET_MIN", None)
os.environ.pop("MLHIP_MSM_BATCH_BUCKET_SLICE", None)
sys.exit(0 if all_same else 1)
