#!/usr/bin/env python3
"""mlhip_gt_exp_device against mlhip_gt_exp_cyclo_device on identical MEMBER inputs: a same-process, interleaved A/B with
device events, on device-resident inputs, per curve, over n in {1, 2^10, 2^14, 2^16} and both MLHIP_PAIRING_QUAD settings
(unset = quads, the default of both entry points; 0 = lane pairs).
Inputs: n members of Gt (one oracle pairing raised to random scalars on the device) and n random 256-bit scalars.
Per cell: two warm-up rounds, then --reps rounds over the four sides (generic / cyclo x quads / pairs) with the order rotated
by one every round, so no side always follows the same other side's kernels; each timed sample is --inner back-to-back
launches between two events (a single launch at n = 1 is a few ms: long enough for events, the inner count steadies it).
Printed: median [min .. max] per launch of each side and the ratio generic / cyclo of the medians for each kernel shape.  The
four outputs of the last round must be byte-equal.
  python tools/perf_gt_exp_cyclo.py --out profiles/gt_exp_cyclo_ab.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mathlib_amd import _lib  # noqa: E402
from oracle import cref  # noqa: E402

CURVES = [("BN254", 0), ("BLS12-381", 1), ("BLS12-377", 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--curves", default="0,1,2")
    ap.add_argument("--sizes", default="1,1024,16384,65536")
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    if _lib.device_count() < 1:
        sys.exit("no GPU: nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/perf_gt_exp_cyclo.py  reps=%d inner=%d  device=%s  source=%s" % (
        args.reps, args.inner, torch.cuda.get_device_name(0), __import__("mathlib_amd.build", fromlist=["x"]).source_hash()))
    emit("# ms per launch: median [min .. max]; ratio = mlhip_gt_exp_device / mlhip_gt_exp_cyclo_device (medians), same kernel shape")
    st = torch.cuda.current_stream().cuda_stream
    sizes = [int(s) for s in args.sizes.split(",")]
    nmax = max(sizes)
    for name, cid in CURVES:
        if str(cid) not in args.curves.split(","):
            continue
        gtsz = 12 * (32 if cid == 0 else 48)
        member = cref.pairing_batch(cid, cref.gen_points(cid, 1, 777, 0, 1), cref.gen_points(cid, 2, 999, 0, 1), 1)
        gen = torch.Generator(device="cpu").manual_seed(1000 + cid)
        base = torch.frombuffer(bytearray(member * nmax), dtype=torch.uint8).cuda()
        sc0 = torch.randint(0, 256, (32 * nmax,), dtype=torch.uint8, generator=gen).cuda()
        sc = torch.randint(0, 256, (32 * nmax,), dtype=torch.uint8, generator=gen).cuda()
        gts = torch.empty(nmax * gtsz, dtype=torch.uint8, device="cuda")
        _lib.check(lib.mlhip_gt_exp_device(cid, base.data_ptr(), sc0.data_ptr(), 0, nmax, gts.data_ptr(), st))  # n members
        torch.cuda.synchronize()
        for n in sizes:
            outs = {}
            sides = []
            for shape, env in (("quads", None), ("pairs", "0")):
                for label, fn in (("generic", lib.mlhip_gt_exp_device), ("cyclo", lib.mlhip_gt_exp_cyclo_device)):
                    key = label + "/" + shape
                    outs[key] = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
                    sides.append((key, fn, env))

            def timed(key, fn, env):
                os.environ.pop("MLHIP_PAIRING_QUAD", None)
                if env is not None:
                    os.environ["MLHIP_PAIRING_QUAD"] = env
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    _lib.check(fn(cid, gts.data_ptr(), sc.data_ptr(), 0, n, outs[key].data_ptr(), st))
                e1.record()
                e1.synchronize()
                os.environ.pop("MLHIP_PAIRING_QUAD", None)
                return e0.elapsed_time(e1) / args.inner

            t = {s[0]: [] for s in sides}
            for r in range(args.reps + 2):
                k = r % len(sides)
                for key, fn, env in sides[k:] + sides[:k]:
                    ms = timed(key, fn, env)
                    if r >= 2:
                        t[key].append(ms)
            torch.cuda.synchronize()
            first = outs[sides[0][0]]
            assert all(torch.equal(first, o) for o in outs.values()), (name, n)
            med = {k: statistics.median(v) for k, v in t.items()}
            s = "%-9s n=%-6d" % (name, n)
            for key, _, _ in sides:
                s += "  %s %.3f [%.3f .. %.3f]" % (key, med[key], min(t[key]), max(t[key]))
            s += "  ratio quads %.3f pairs %.3f" % (med["generic/quads"] / med["cyclo/quads"], med["generic/pairs"] / med["cyclo/pairs"])
            emit(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
