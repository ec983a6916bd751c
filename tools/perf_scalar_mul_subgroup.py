#!/usr/bin/env python3
"""mlhip_scalar_mul_device with MLHIP_GROUP_SUBGROUP against the plain call on identical inputs: a same-process, interleaved
A/B with device events on device-resident inputs -- three curves x two groups x n in {2^10, 2^14, 2^16, 2^20}, one point per
scalar (point_stride 1).
Inputs: n points of the prime-order subgroup ([k_i]G from the library's fixed-base path) and n random 256-bit scalars.
Per cell: two warm-up rounds, then --reps rounds over three sides -- flagged, plain, and plain a SECOND time into its own
buffer -- with the order rotated by one every round, so no side always follows the same other side's kernels; each timed
sample is `inner` back-to-back launches between two events (3 below 2^16 products, 1 from there on).
Printed: median [min .. max] per launch of each side; ratio = flagged / plain (medians); spread = |plain - plain again| /
plain (medians): what two identical runs of the same call differ by in this process; the verdict `ahead` needs
1 - ratio > spread.  The three outputs of the last round must be byte-equal.
`counted` is the ratio the operation counts of DESIGN.md sections 17 and 20 predict.
  python tools/perf_scalar_mul_subgroup.py --ab --out profiles/scalar_mul_endo_ab.txt
  python tools/perf_scalar_mul_subgroup.py --ab --curves 0 --groups 1 --out profiles/scalar_mul_glv_ab.txt   (the lattice split of BN254 G1)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mathlib_amd import _lib  # noqa: E402
from oracle import cref  # noqa: E402

CURVES = [("BN254", 0), ("BLS12-381", 1), ("BLS12-377", 2)]
# flagged / plain as the operation counts predict it, by (BN254?, group)
COUNTED = {(True, 1): 0.66, (False, 1): 0.67, (True, 2): 0.65, (False, 2): 0.5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true", help="the A/B (the only mode)")
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="0,1,2")
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--sizes", default="1024,16384,65536,1048576")
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    if _lib.device_count() < 1:
        sys.exit("no GPU: nothing is measured without one")
    for name in ("MLHIP_SCALAR_MUL_ENDO", "MLHIP_FIXED_BASE_MIN", "MLHIP_SCALAR_MUL_ONE_LANE"):
        os.environ.pop(name, None)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/perf_scalar_mul_subgroup.py --ab  reps=%d  device=%s  source=%s" % (
        args.reps, torch.cuda.get_device_name(0), __import__("mathlib_amd.build", fromlist=["x"]).source_hash()))
    emit("# ms per launch of mlhip_scalar_mul_device, point_stride 1: median [min .. max]; ratio = flagged / plain; spread = |plain - plain again| / plain")
    st = torch.cuda.current_stream().cuda_stream
    sizes = [int(s) for s in args.sizes.split(",")]
    nmax = max(sizes)
    for name, cid in CURVES:
        if str(cid) not in args.curves.split(","):
            continue
        fpb = 32 if cid == 0 else 48
        for group in (1, 2):
            if str(group) not in args.groups.split(","):
                continue
            psz = 2 * group * fpb
            gen = torch.Generator(device="cpu").manual_seed(3000 + 10 * cid + group)
            base = torch.frombuffer(bytearray(cref.gen_points(cid, group, 777, 0, 1)), dtype=torch.uint8).cuda()
            sc0 = torch.randint(0, 256, (32 * nmax,), dtype=torch.uint8, generator=gen).cuda()
            sc = torch.randint(0, 256, (32 * nmax,), dtype=torch.uint8, generator=gen).cuda()
            pts = torch.empty(nmax * psz, dtype=torch.uint8, device="cuda")
            _lib.check(lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, sc0.data_ptr(), 0, nmax, pts.data_ptr(), st))  # n points of the subgroup
            torch.cuda.synchronize()
            for n in sizes:
                inner = 3 if n < (1 << 16) else 1
                sides = [("flagged", _lib.GROUP_SUBGROUP(group)), ("plain", group), ("plain again", group)]
                outs = {key: torch.empty(n * psz, dtype=torch.uint8, device="cuda") for key, _ in sides}

                def timed(key, g):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(inner):
                        _lib.check(lib.mlhip_scalar_mul_device(cid, g, pts.data_ptr(), 1, sc.data_ptr(), 0, n, outs[key].data_ptr(), st))
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) / inner

                t = {key: [] for key, _ in sides}
                for r in range(args.reps + 2):
                    k = r % len(sides)
                    for key, g in sides[k:] + sides[:k]:
                        ms = timed(key, g)
                        if r >= 2:
                            t[key].append(ms)
                torch.cuda.synchronize()
                equal = all(torch.equal(outs["plain"], o) for o in outs.values())
                med = {k: statistics.median(v) for k, v in t.items()}
                ratio = med["flagged"] / med["plain"]
                spread = abs(med["plain"] - med["plain again"]) / med["plain"]
                s = "%-9s G%d n=%-8d" % (name, group, n)
                for key, _ in sides:
                    s += "  %s %.3f [%.3f .. %.3f]" % (key, med[key], min(t[key]), max(t[key]))
                verdict = "ahead" if 1.0 - ratio > spread else "NOT AHEAD"
                s += "  ratio %.3f  counted %.2f  spread %.4f  %s  bytes %s" % (ratio, COUNTED[cid == 0, group], spread, verdict,
                                                                                 "equal" if equal else "DIFFER")
                emit(s)
                assert equal, (name, group, n)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
