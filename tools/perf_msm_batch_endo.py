#!/usr/bin/env python3
"""A/B of the endomorphism-split Straus chunks of mlhip_msm_batch* (mathlib_amd/csrc/msm_batch_endo.h) on one GPU, in one
process: the device form between events, the call flagged with MLHIP_CURVE_SUBGROUP_POINTS against the plain call on the same
device buffers, and the plain call against itself for the spread.

  --ab     three sides per cell -- flagged, plain, plain again -- interleaved in rotating order, medians of 7 timed rounds
           after 2 warm-up rounds, the outputs of all three compared byte for byte in every cell
  grid     the three curves x G1, G2 x chunk length P in {1, 2, 4, 8} (MLHIP_MSM_BATCH_CHUNK) x segment length m in
           {2, 4, 16, 64} x segment count K in {2^10, 2^14, 2^16}; points [s_i]G of the subgroup, uniform 256-bit scalars
  rule     a (curve, group) takes the split route by default only if the flagged call is ahead of the plain call by more than
           the plain / plain spread in EVERY cell at the default P; the default P for flagged calls is the P with the best
           median of flagged time over the grid (geometric mean over the cells).  The tool prints both per (curve, group).

Every cell runs under a time limit: a cell that passes it ends the run.

Usage: perf_msm_batch_endo.py --ab [--out FILE] [--rounds N] [--warmup N] [--step-limit SECONDS] [--curves A,B] [--groups 1,2]
                                   [--chunks 1,2,4,8] [--max-k LOG2]
       perf_msm_batch_endo.py --ab --curves BN254 --groups 1 --out profiles/msm_batch_glv_ab.txt   (the lattice split of BN254 G1)"""
import argparse
import math
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

M_GRID = (2, 4, 16, 64)
K_GRID = (1 << 10, 1 << 14, 1 << 16)
DEFAULT_P = {1: 4, 2: 4}  # MSM_BATCH_P_DEFAULT_G1 / _G2
# operations per pair, counted from the code: (doublings per chunk, table operations per pair, additions per pair at most)
PLAIN = (256, 7, 64)
SPLIT = {("BLS12", 1): (128, 7, 66), ("BLS12", 2): (64, 11, 64), ("BN", 1): (128, 7, 66), ("BN", 2): (128, 13, 64)}

ap = argparse.ArgumentParser()
ap.add_argument("--ab", action="store_true", required=True)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_batch_endo_ab.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-limit", type=int, default=120)
ap.add_argument("--curves", default="BN254,BLS12-381,BLS12-377")
ap.add_argument("--groups", default="1,2")
ap.add_argument("--chunks", default="1,2,4,8")
ap.add_argument("--max-k", type=int, default=16)
args = ap.parse_args()

lib = _lib.load()
assert _lib.device_count() >= 1, "no GPU: nothing to measure"
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
st = stream.cuda_stream
gen = torch.Generator(device=dev)
gen.manual_seed(19)
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def save():
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def step_limit(signum, frame):
    save()
    raise SystemExit("a cell passed its time limit of %d s: the run ends here" % args.step_limit)


signal.signal(signal.SIGALRM, step_limit)


def rnd_scalars(k):
    return torch.randint(-(1 << 63), (1 << 63) - 1, (k, 4), dtype=torch.int64, generator=gen, device=dev).view(torch.uint8).reshape(-1).contiguous()


def predicted(name, group, P):
    fam = "BN" if name == "BN254" else "BLS12"
    if (fam, group) not in SPLIT:
        return 1.0
    cost = lambda c: c[0] / P + c[1] + c[2]
    return cost(SPLIT[fam, group]) / cost(PLAIN)


def run_cell(cid, group, psz, pts, scs, K, m):
    """(median ms of flagged, plain, plain again; all outputs equal)"""
    signal.alarm(args.step_limit)
    offs = _lib.batch_offsets([m] * K)
    sides = [(c, [], torch.zeros(K * psz, dtype=torch.uint8, device=dev)) for c in (_lib.CURVE_SUBGROUP_POINTS(cid), cid, cid)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup + args.rounds):
        for i in range(3):
            curve_arg, ms, out = sides[(i + r) % 3]
            e0.record(stream)
            rc = lib.mlhip_msm_batch_device(curve_arg, group, pts.data_ptr(), scs.data_ptr(), 0, offs, K, out.data_ptr(), st)
            e1.record(stream)
            assert rc == 0, (rc, curve_arg)
            e1.synchronize()
            if r >= args.warmup:
                ms.append(e0.elapsed_time(e1))
    same = all(torch.equal(sides[0][2], sd[2]) for sd in sides[1:])
    signal.alarm(0)
    return [statistics.median(sd[1]) for sd in sides], same


emit("# endomorphism-split Straus chunks of mlhip_msm_batch_device against the plain chunks: tools/perf_msm_batch_endo.py --ab")
emit("# source %s, device %s, medians of %d timed rounds per cell after %d warm-up rounds, three sides interleaved in rotating" %
     (source_hash(), torch.cuda.get_device_name(0), args.rounds, args.warmup))
emit("# order (flagged, plain, plain again), device form between events; ratio = flagged / plain, spread = |plain - plain'| / plain")
all_same = True
verdicts = []
chunks = [int(v) for v in args.chunks.split(",")]
k_grid = [k for k in K_GRID if k <= 1 << args.max_k]
for name in args.curves.split(","):
    g = load_golden(name)
    cid = g["curve_id"]
    _, g1b, g2b, _ = _lib.sizes(cid)
    for group in [int(v) for v in args.groups.split(",")]:
        psz = g1b if group == 1 else g2b
        nmax = max(k_grid) * max(M_GRID)
        # 4096 distinct points [s_i] G of the subgroup, repeated: the cost of a pair does not depend on the point
        signal.alarm(args.step_limit)
        base = torch.frombuffer(bytearray(bytes.fromhex(g["g1_gen" if group == 1 else "g2_gen"])), dtype=torch.uint8).to(dev)
        distinct = torch.empty(4096 * psz, dtype=torch.uint8, device=dev)
        _lib.check(lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, rnd_scalars(4096).data_ptr(), 0, 4096, distinct.data_ptr(), st))
        pts = distinct.repeat(nmax // 4096).contiguous()
        scs = rnd_scalars(nmax)
        torch.cuda.synchronize()
        signal.alarm(0)
        emit()
        emit("## %s G%d" % (name, group))
        emit("%3s %7s %4s %11s %10s %10s %7s %7s %7s %6s" % ("P", "K", "m", "flagged ms", "plain ms", "plain' ms", "ratio", "spread", "counted", "equal"))
        cells = {}
        for P in chunks:
            os.environ["MLHIP_MSM_BATCH_CHUNK"] = str(P)
            for K in k_grid:
                for m in M_GRID:
                    (f, p0, p1), same = run_cell(cid, group, psz, pts, scs, K, m)
                    all_same &= same
                    spread = abs(p0 - p1) / p0
                    cells[P, K, m] = (f, p0, spread)
                    emit("%3d %7d %4d %11.3f %10.3f %10.3f %7.3f %7.3f %7.2f %6s" % (P, K, m, f, p0, p1, f / p0, spread, predicted(name, group, P), same))
            save()
        os.environ.pop("MLHIP_MSM_BATCH_CHUNK", None)
        geo = {P: math.exp(statistics.mean(math.log(cells[P, K, m][0]) for K in k_grid for m in M_GRID)) for P in chunks}
        geo_plain = {P: math.exp(statistics.mean(math.log(cells[P, K, m][1]) for K in k_grid for m in M_GRID)) for P in chunks}
        best = min(geo, key=geo.get)
        dp = DEFAULT_P[group]
        line = "## %s G%d: geometric mean over the cells, flagged ms by P: %s; plain: %s; best flagged P = %d" % (
            name, group, " ".join("%d:%.3f" % (P, geo[P]) for P in chunks), " ".join("%d:%.3f" % (P, geo_plain[P]) for P in chunks), best)
        emit(line)
        if dp in chunks:
            at = [(K, m) + cells[dp, K, m] for K in k_grid for m in M_GRID]
            behind = [(K, m) for K, m, f, p0, spread in at if not f < p0 * (1 - spread)]
            ratios = [f / p0 for K, m, f, p0, spread in at]
            verdict = "%s G%d at P = %d: ratio %.3f .. %.3f, largest spread %.3f, ahead by more than the spread in %d of %d cells%s" % (
                name, group, dp, min(ratios), max(ratios), max(c[4] for c in at), len(at) - len(behind), len(at),
                "" if not behind else "; not in (K, m) = %s" % behind)
            verdicts.append(verdict)
            emit("## " + verdict)
emit()
emit("# all outputs byte-equal: %s" % all_same)
for v in verdicts:
    emit("# " + v)
save()
sys.exit(0 if all_same else 1)
