#!/usr/bin/env python3
"""The Gt wire codec, the membership test and Gt.Inverse on device-resident inputs, with mlhip_gt_exp_cyclo_device on the same
member inputs as the yardstick: a same-process, interleaved measurement with device events, per curve, over n in {1, 2^10,
2^14, 2^16} and both MLHIP_PAIRING_QUAD settings (unset = quads, the default; 0 = lane pairs -- the codec kernels proper have
one shape, the checking decoder's second launch has two).
Inputs: n members of Gt (one oracle pairing raised to random scalars on the device), their encodings, n random scalars.
Per cell: two warm-up rounds, then --reps rounds over the sides with the order rotated by one every round, so no side always
follows the same other side's kernels; each timed sample is --inner back-to-back launches between two events.
Printed: median [min .. max] ms per launch of each side.  Every status of the last round must be 0 and the decoders must give
the inputs back.
  python tools/perf_gt_codec.py --out profiles/gt_codec_ab.txt"""
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

    emit("# tools/perf_gt_codec.py  reps=%d inner=%d  device=%s  source=%s" % (
        args.reps, args.inner, torch.cuda.get_device_name(0), __import__("mathlib_amd.build", fromlist=["x"]).source_hash()))
    emit("# ms per launch: median [min .. max]; member inputs; exp_cyclo = mlhip_gt_exp_cyclo_device on the same inputs")
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
        wire = torch.empty(nmax * gtsz, dtype=torch.uint8, device="cuda")
        _lib.check(lib.mlhip_gt_exp_device(cid, base.data_ptr(), sc0.data_ptr(), 0, nmax, gts.data_ptr(), st))  # n members
        _lib.check(lib.mlhip_gt_to_bytes_device(cid, gts.data_ptr(), nmax, wire.data_ptr(), st))
        torch.cuda.synchronize()
        for n in sizes:
            out = {}
            status = {}
            sides = []
            for shape, env in (("quads", None), ("pairs", "0")):
                for label in ("is_member", "from_bytes/0", "from_bytes/1", "to_bytes", "inverse", "exp_cyclo"):
                    key = label + " " + shape
                    out[key] = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
                    status[key] = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
                    sides.append((key, label, env))

            def launch(key, label):
                o, s = out[key].data_ptr(), status[key].data_ptr()
                if label == "is_member":
                    return lib.mlhip_gt_is_member_device(cid, gts.data_ptr(), n, s, st)
                if label.startswith("from_bytes"):
                    return lib.mlhip_gt_from_bytes_device(cid, wire.data_ptr(), n, int(label[-1]), o, s, st)
                if label == "to_bytes":
                    return lib.mlhip_gt_to_bytes_device(cid, gts.data_ptr(), n, o, st)
                if label == "inverse":
                    return lib.mlhip_gt_inverse_device(cid, gts.data_ptr(), n, o, st)
                return lib.mlhip_gt_exp_cyclo_device(cid, gts.data_ptr(), sc.data_ptr(), 0, n, o, st)

            def timed(key, label, env):
                os.environ.pop("MLHIP_PAIRING_QUAD", None)
                if env is not None:
                    os.environ["MLHIP_PAIRING_QUAD"] = env
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    _lib.check(launch(key, label))
                e1.record()
                e1.synchronize()
                os.environ.pop("MLHIP_PAIRING_QUAD", None)
                return e0.elapsed_time(e1) / args.inner

            t = {s[0]: [] for s in sides}
            for r in range(args.reps + 2):
                k = r % len(sides)
                for key, label, env in sides[k:] + sides[:k]:
                    ms = timed(key, label, env)
                    if r >= 2:
                        t[key].append(ms)
            torch.cuda.synchronize()
            for key, label, _ in sides:
                if label == "is_member" or label.startswith("from_bytes"):
                    assert not status[key].any().item(), (name, n, key)
                if label.startswith("from_bytes"):
                    assert torch.equal(out[key], gts[: n * gtsz]), (name, n, key)
                if label == "to_bytes":
                    assert torch.equal(out[key], wire[: n * gtsz]), (name, n, key)
            for shape in ("quads", "pairs"):
                s = "%-9s n=%-6d %s" % (name, n, shape)
                for key, label, _ in sides:
                    if key.endswith(shape):
                        s += "  %s %.3f [%.3f .. %.3f]" % (label, statistics.median(t[key]), min(t[key]), max(t[key]))
                emit(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
