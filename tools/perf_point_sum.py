#!/usr/bin/env python3
"""mlhip_g1_sum / mlhip_g2_sum: host loop (MLHIP_SUM_DEVICE_MIN=0) against device route (=1), both through the host-buffer
call -- the upload over PCIe is part of the device side -- in one process, interleaved, on one GPU: G1 and G2 of the three
curves, n = 2^6 .. 2^22 in steps of 4x.
Inputs: 2^16 + 1 distinct points (cref.gen_points), repeated to n (no lane or lane pair ever meets the same point twice: the
period is odd, the lane counts are powers of two), in pageable host memory as a caller's would be.
Per cell: one warm-up call of the device route (the host loop has nothing to warm), then rounds of (host, device) or
(device, host), alternating, until each route has run for --min-seconds and at least --reps times (at most --max-reps; two
rounds where one round takes over two seconds); wall clock around the call, which returns after its download.  Printed: median [min .. max] ms per call of each route and host / device.  The two routes must agree byte for byte
in every cell.  Last: per group, the smallest n from which the device route is ahead at every larger measured size on every
curve -- the default of MLHIP_SUM_DEVICE_MIN (the grid is powers of two, so it is one already).
  python tools/perf_point_sum.py --out profiles/point_sum_ab.txt"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mathlib_amd import _lib  # noqa: E402
from oracle import cref  # noqa: E402

CURVES = [("BN254", 0, 32), ("BLS12-381", 1, 48), ("BLS12-377", 2, 48)]
PERIOD = (1 << 16) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-reps", type=int, default=25)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    ap.add_argument("--curves", default="0,1,2")
    ap.add_argument("--log2", default="6,8,10,12,14,16,18,20,22")
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    if _lib.device_count() < 1:
        sys.exit("no GPU: nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/perf_point_sum.py  reps>=%d min_seconds=%.2f  device=%s  source=%s" % (
        args.reps, args.min_seconds, torch.cuda.get_device_name(0), __import__("mathlib_amd.build", fromlist=["x"]).source_hash()))
    emit("# ms per host-buffer call (upload and download included): median [min .. max] (calls); host = MLHIP_SUM_DEVICE_MIN=0, device = 1")
    sizes = [1 << int(s) for s in args.log2.split(",")]
    ahead = {1: {}, 2: {}}  # group -> n -> device ahead on every curve measured
    for name, cid, fpb in CURVES:
        if str(cid) not in args.curves.split(","):
            continue
        for group in (1, 2):
            ps = 2 * group * fpb
            block = cref.gen_points(cid, group, 0xA11CE + group, 0xB0B + cid, PERIOD)
            pts = (block * (max(sizes) // PERIOD + 1))[: max(sizes) * ps]
            fn = lib.mlhip_g1_sum if group == 1 else lib.mlhip_g2_sum
            out = {"0": ctypes.create_string_buffer(ps), "1": ctypes.create_string_buffer(ps)}

            def call(route, n):
                os.environ["MLHIP_SUM_DEVICE_MIN"] = route
                t0 = time.perf_counter()
                rc = fn(cid, pts, n, out[route])
                dt = time.perf_counter() - t0
                _lib.check(rc)
                return dt

            for n in sizes:
                t = {"0": [], "1": []}
                call("1", n)  # warm-up: code objects, the lease's arena, the sum scratch
                r = 0
                while r < args.max_reps and (r < args.reps or min(sum(t["0"]), sum(t["1"])) < args.min_seconds):
                    if r >= 2 and t["0"][0] + t["1"][0] > 2.0:
                        break
                    for route in ("0", "1") if r % 2 == 0 else ("1", "0"):
                        t[route].append(call(route, n))
                    r += 1
                assert out["0"].raw == out["1"].raw and any(out["0"].raw), (name, group, n)
                h, d = statistics.median(t["0"]), statistics.median(t["1"])
                ahead[group][n] = ahead[group].get(n, True) and d * 1.04 < h  # ahead by more than the spread between boxes
                emit("%-9s G%d n=2^%-2d  host %10.3f [%10.3f .. %10.3f]  device %8.3f [%8.3f .. %8.3f]  (%2d)  host/device %7.2f" % (
                    name, group, n.bit_length() - 1, h * 1e3, min(t["0"]) * 1e3, max(t["0"]) * 1e3, d * 1e3, min(t["1"]) * 1e3,
                    max(t["1"]) * 1e3, r, h / d))
    os.environ.pop("MLHIP_SUM_DEVICE_MIN", None)
    for group in (1, 2):
        best = None
        for n in sorted(ahead[group], reverse=True):
            if not ahead[group][n]:
                break
            best = n
        emit("# G%d: device route ahead at every measured size from %s on -> default MLHIP_SUM_DEVICE_MIN %s" % (
            group, "2^%d" % (best.bit_length() - 1) if best else "nowhere", "2^%d" % (best.bit_length() - 1) if best else "none (host loop)"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
