#!/usr/bin/env python3
"""A/B of the segmented point sums (mathlib_amd/csrc/msm_sum_batch.h: the batch calls with MLHIP_SCALARS_UNIT) on one GPU, in
one process: mlhip_sum_batch_device against mlhip_msm_batch_device with a resident array of plain-integer ones -- the only
device route there was before -- on the same device buffers, and the plain call against itself for the spread.

  sides    per cell: flagged at the default S, plain, plain again, flagged at S = 4, 8, 16, 32 (MLHIP_SUM_BATCH_SLICE) --
           interleaved in rotating order, medians of the timed rounds after the warm-up rounds, device form between events,
           the outputs of all sides compared byte for byte in every cell
  grid     K in {2^10, 2^14, 2^16} x points per segment m in {2, 16, 64, 512, 4096} with K m <= 2^22, BLS12-381 G1 and G2; one
           BN254 G1 column (K = 2^14); one row over a 4096-base handle with a random index list (K = 2^14; the plain side is
           mlhip_bases_msm_batch_device with ones); one cell of the host form against K host mlhip_g1_sum calls
  counted  ~9 group operations per point for the plain call (the {1..8} P table and one addition), 1 + 1.4 / S for the flagged
  rule     sum_batch_slice_default of msm_sum_batch.h: the largest S in {4, 8, 16, 32} with total / S >= 2^13.  The tool prints,
           per cell, the best S and the rule's S, and lists the cells where another S beats the rule's by more than 5 %

Every cell runs under a time limit: a cell that passes it ends the run.

Usage: perf_sum_batch.py [--out FILE] [--rounds N] [--warmup N] [--step-limit SECONDS] [--max-total LOG2]"""
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

K_GRID = (1 << 10, 1 << 14, 1 << 16)
M_GRID = (2, 16, 64, 512, 4096)
S_GRID = (4, 8, 16, 32)
FILL = 1 << 13  # SUM_BATCH_FILL_SLICES (below POINT_SUM_MAX_LANES_G1 / _G2, so the same for both groups)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_batch_ab.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-limit", type=int, default=120)
ap.add_argument("--max-total", type=int, default=22)
args = ap.parse_args()

lib = _lib.load()
assert _lib.device_count() >= 1, "no GPU: nothing to measure"
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
st = stream.cuda_stream
gen = torch.Generator(device=dev)
gen.manual_seed(23)
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


def rule_s(total, group):
    """sum_batch_slice_default of msm_sum_batch.h"""
    for S in (32, 16, 8):
        if total // S >= FILL:
            return S
    return 4


def rnd_scalars(k):
    return torch.randint(-(1 << 63), (1 << 63) - 1, (k, 4), dtype=torch.int64, generator=gen, device=dev).view(torch.uint8).reshape(-1).contiguous()


def ones(n):
    t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    t[:, 0] = 1
    return t.reshape(-1).contiguous()


def run_cell(flagged, plain, psz, K):
    """flagged(out_ptr), plain(out_ptr) queue one call on the stream.  (median ms of [flagged default, plain, plain again,
    flagged at each S of S_GRID]; all outputs equal)"""
    signal.alarm(args.step_limit)
    sides = [(None, flagged), (None, plain), (None, plain)] + [(S, flagged) for S in S_GRID]
    outs = [torch.zeros(K * psz, dtype=torch.uint8, device=dev) for _ in sides]
    ms = [[] for _ in sides]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup + args.rounds):
        for i in range(len(sides)):
            j = (i + r) % len(sides)
            S, call = sides[j]
            if S is None:
                os.environ.pop("MLHIP_SUM_BATCH_SLICE", None)
            else:
                os.environ["MLHIP_SUM_BATCH_SLICE"] = str(S)
            e0.record(stream)
            rc = call(outs[j].data_ptr())
            e1.record(stream)
            assert rc == 0, (rc, j, lib.mlhip_last_error())
            e1.synchronize()
            if r >= args.warmup:
                ms[j].append(e0.elapsed_time(e1))
    os.environ.pop("MLHIP_SUM_BATCH_SLICE", None)
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    signal.alarm(0)
    return [statistics.median(m) for m in ms], same


HEAD = "%7s %5s %11s %10s %10s %7s %7s %8s  %s  %6s %5s %6s" % (
    "K", "m", "flagged ms", "plain ms", "plain' ms", "ratio", "spread", "counted", "  ".join("S=%-2d ms " % S for S in S_GRID), "best S", "rule", "equal")
all_same = True
behind = []
rule_beaten = []


def report(label, K, m, group, med, same):
    global all_same
    f, p0, p1 = med[:3]
    by_s = dict(zip(S_GRID, med[3:]))
    spread = abs(p0 - p1) / p0
    best = min(by_s, key=by_s.get)
    rs = rule_s(K * m, group)
    all_same &= same
    if not f < p0 * (1 - spread):
        behind.append("%s K=%d m=%d: flagged %.3f ms, plain %.3f ms, spread %.3f" % (label, K, m, f, p0, spread))
    if m > min(S_GRID) and by_s[best] < by_s[rs] * 0.95:  # (m <= 4: one slice per segment at every S)
        rule_beaten.append("%s K=%d m=%d: S=%d %.3f ms against the rule's S=%d %.3f ms" % (label, K, m, best, by_s[best], rs, by_s[rs]))
    emit("%7d %5d %11.3f %10.3f %10.3f %7.3f %7.3f %8.3f  %s  %6d %5d %6s" % (
        K, m, f, p0, p1, f / p0, spread, (1 + 1.4 / rs) / 9.0, "  ".join("%8.3f" % by_s[S] for S in S_GRID), best, rs, same))


def make_points(cid, group, psz, g, n):
    """4096 distinct points [s_i] G of the subgroup, repeated: the cost of an addition does not depend on the point"""
    base = torch.frombuffer(bytearray(bytes.fromhex(g["g1_gen" if group == 1 else "g2_gen"])), dtype=torch.uint8).to(dev)
    distinct = torch.empty(4096 * psz, dtype=torch.uint8, device=dev)
    _lib.check(lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, rnd_scalars(4096).data_ptr(), 0, 4096, distinct.data_ptr(), st))
    torch.cuda.synchronize()
    return distinct, distinct.repeat(max(1, n // 4096)).contiguous()


emit("# segmented point sums against mlhip_msm_batch_device with a resident array of ones: tools/perf_sum_batch.py")
emit("# source %s, device %s, medians of %d timed rounds per cell after %d warm-up rounds, the sides interleaved in rotating" %
     (source_hash(), torch.cuda.get_device_name(0), args.rounds, args.warmup))
emit("# order, device form between events; ratio = flagged / plain, spread = |plain - plain'| / plain, counted = (1 + 1.4 / S) / 9")
max_total = 1 << args.max_total
for name, group, k_grid in (("BLS12-381", 1, K_GRID), ("BLS12-381", 2, K_GRID), ("BN254", 1, (1 << 14,))):
    g = load_golden(name)
    cid = g["curve_id"]
    _, g1b, g2b, _ = _lib.sizes(cid)
    psz = g1b if group == 1 else g2b
    signal.alarm(args.step_limit)
    nmax = max(K * m for K in k_grid for m in M_GRID if K * m <= max_total)
    distinct, pts = make_points(cid, group, psz, g, nmax)
    scs = ones(nmax)
    torch.cuda.synchronize()
    signal.alarm(0)
    emit()
    emit("## %s G%d" % (name, group))
    emit(HEAD)
    for K in k_grid:
        for m in M_GRID:
            if K * m > max_total:
                continue
            offs = _lib.batch_offsets([m] * K)
            med, same = run_cell(
                lambda o: _lib.mlhip_sum_batch_device(lib, cid, group, pts.data_ptr(), offs, K, o, st),
                lambda o: lib.mlhip_msm_batch_device(cid, group, pts.data_ptr(), scs.data_ptr(), 0, offs, K, o, st), psz, K)
            report("%s G%d" % (name, group), K, m, group, med, same)
        save()
    if (name, group) == ("BLS12-381", 1):
        # one row over a 4096-base handle with an index list
        emit()
        emit("## %s G1, a 4096-base handle with a random index list (plain: mlhip_bases_msm_batch_device with ones)" % name)
        emit(HEAD)
        h = ctypes.c_void_p()
        _lib.check(lib.mlhip_bases_create_device(cid, group, distinct.data_ptr(), 4096, 0, ctypes.byref(h)))
        K = 1 << 14
        for m in (2, 16, 64):
            offs = _lib.batch_offsets([m] * K)
            idx_t = torch.randint(0, 4096, (K * m,), dtype=torch.int32, generator=gen, device=dev).cpu().numpy().astype("uint32")
            idx = idx_t.ctypes.data_as(ctypes.c_void_p)
            med, same = run_cell(
                lambda o: _lib.mlhip_bases_sum_batch_device(lib, h, idx, offs, K, st, o),
                lambda o: lib.mlhip_bases_msm_batch_device(h, scs.data_ptr(), 0, idx, offs, K, st, o), psz, K)
            report("%s G1 handle" % name, K, m, group, med, same)
        torch.cuda.synchronize()
        lib.mlhip_bases_destroy(h)
        # one cell of the host form against K host mlhip_g1_sum calls (below MLHIP_SUM_DEVICE_MIN: the one-core host loop)
        signal.alarm(args.step_limit)
        K, m = 1 << 10, 64
        host_pts = bytes(pts[: K * m * psz].cpu().numpy().tobytes())
        offs = _lib.batch_offsets([m] * K)
        out_b = ctypes.create_string_buffer(K * psz)
        out_s = ctypes.create_string_buffer(K * psz)
        t_batch, t_single = [], []
        for r in range(args.warmup + args.rounds):
            t0 = time.perf_counter()
            _lib.check(_lib.mlhip_sum_batch(lib, cid, group, host_pts, offs, K, out_b))
            t1 = time.perf_counter()
            for s in range(K):
                _lib.check(lib.mlhip_g1_sum(cid, host_pts[s * m * psz : (s + 1) * m * psz], m, ctypes.byref(out_s, s * psz)))
            t2 = time.perf_counter()
            if r >= args.warmup:
                t_batch.append(1e3 * (t1 - t0))
                t_single.append(1e3 * (t2 - t1))
        signal.alarm(0)
        same = out_b.raw == out_s.raw
        all_same &= same
        emit()
        emit("## %s G1 host form, K = %d segments of %d points: one mlhip_sum_batch call %.3f ms, K mlhip_g1_sum calls %.3f ms, ratio %.3f, equal %s" % (
            name, K, m, statistics.median(t_batch), statistics.median(t_single), statistics.median(t_batch) / statistics.median(t_single), same))
        save()
    del pts, scs
    torch.cuda.empty_cache()
emit()
emit("# all outputs byte-equal: %s" % all_same)
emit("# cells where the flagged call is not ahead of the plain call by more than the spread: %s" % (behind or "none"))
emit("# cells where another S beats the rule's S by more than 5 %%: %s" % (rule_beaten or "none"))
save()
sys.exit(0 if all_same else 1)
