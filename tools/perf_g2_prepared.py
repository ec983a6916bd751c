#!/usr/bin/env python3
"""Prepared G2 handles against the general entry points: a same-process, interleaved A/B with device events, on
device-resident inputs, per curve, over ppp in {1, 2} x n_products in {1, 2^10, 2^14, 2^16}:
  miller   mlhip_miller_loop_device                         vs  mlhip_miller_loop_prepared_device
  pairing  mlhip_miller_loop_device + mlhip_final_exp_device vs  mlhip_pairing_prepared_device
Per cell: two warm-up rounds, then --reps rounds of A, B, A, B ... with the order of the sides rotated by one every round (no
side always follows the same other side's kernels); the median and the spread (min .. max) of each side and the ratio
general / prepared of the medians.  The outputs of the two sides of BOTH pairs are compared after the final exponentiation.
Also the time to create a handle of two points (wall clock, median of 5).
--families adds, per cell, the prepared side with the quads forced / forbidden and the fallback (general kernels on expanded
Qs) forced: the numbers the dispatcher's switches rest on.
  python tools/perf_g2_prepared.py --out profiles/g2_prepared_ab.txt"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mathlib_amd import _lib  # noqa: E402
from oracle import cref  # noqa: E402

CURVES = [("BN254", 0), ("BLS12-381", 1), ("BLS12-377", 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--curves", default="0,1,2")
    ap.add_argument("--sizes", default="1,1024,16384,65536")
    ap.add_argument("--families", action="store_true")
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/perf_g2_prepared.py  reps=%d  device=%s  source=%s" % (args.reps, torch.cuda.get_device_name(0),
                                                                      __import__("mathlib_amd.build", fromlist=["x"]).source_hash()))
    emit("# times in ms: median [min .. max]; ratio = general / prepared (medians)")
    st = torch.cuda.current_stream().cuda_stream
    nmax = max(int(s) for s in args.sizes.split(","))
    for name, cid in CURVES:
        if str(cid) not in args.curves.split(","):
            continue
        fpb = 32 if cid == 0 else 48
        g1sz, g2sz, gtsz = 2 * fpb, 4 * fpb, 12 * fpb
        qb = cref.gen_points(cid, 2, 12345, 999, 2)
        walls = []
        for _ in range(5):
            h = ctypes.c_void_p()
            t0 = time.perf_counter()
            _lib.check(lib.mlhip_g2_prepared_create(cid, qb, 2, ctypes.byref(h)))
            walls.append((time.perf_counter() - t0) * 1e3)
            lib.mlhip_g2_prepared_destroy(h)
        emit("%-9s handle of 2 points: create %.3f ms (median of 5, wall clock)" % (name, statistics.median(walls)))
        h = ctypes.c_void_p()
        _lib.check(lib.mlhip_g2_prepared_create(cid, qb, 2, ctypes.byref(h)))
        g1 = torch.frombuffer(bytearray(cref.gen_points(cid, 1, 777, 31, 2 * nmax)), dtype=torch.uint8).cuda()
        for ppp in (1, 2):
            for n in [int(s) for s in args.sizes.split(",")]:
                g2 = torch.frombuffer(bytearray(qb[: ppp * g2sz] * n), dtype=torch.uint8).cuda()
                raw = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
                oa = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
                ob = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")

                def gen_miller():
                    _lib.check(lib.mlhip_miller_loop_device(cid, g1.data_ptr(), g2.data_ptr(), ppp, n, raw.data_ptr(), st))

                def prep_miller():
                    _lib.check(lib.mlhip_miller_loop_prepared_device(h, g1.data_ptr(), None, ppp, n, ob.data_ptr(), st))

                def gen_pairing():
                    _lib.check(lib.mlhip_miller_loop_device(cid, g1.data_ptr(), g2.data_ptr(), ppp, n, raw.data_ptr(), st))
                    _lib.check(lib.mlhip_final_exp_device(cid, raw.data_ptr(), n, oa.data_ptr(), st))

                def prep_pairing():
                    _lib.check(lib.mlhip_pairing_prepared_device(h, g1.data_ptr(), None, ppp, n, ob.data_ptr(), st))

                def timed(fn, env=None):
                    for k in ("MLHIP_PAIRING_QUAD", "MLHIP_G2_PREPARED_GENERAL"):
                        os.environ.pop(k, None)
                    os.environ.update(env or {})
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    for k in env or {}:
                        os.environ.pop(k, None)
                    return e0.elapsed_time(e1)

                for what, fa, fb in (("miller", gen_miller, prep_miller), ("pairing", gen_pairing, prep_pairing)):
                    sides = [("general", fa, None), ("prepared", fb, None)]
                    if args.families:
                        sides += [("prep/quad", fb, {"MLHIP_PAIRING_QUAD": "1", "MLHIP_G2_PREPARED_GENERAL": "0"}),
                                  ("prep/pairs", fb, {"MLHIP_PAIRING_QUAD": "0", "MLHIP_G2_PREPARED_GENERAL": "0"}),
                                  ("prep/fallback", fb, {"MLHIP_G2_PREPARED_GENERAL": "1"})]
                    t = {s[0]: [] for s in sides}
                    for r in range(args.reps + 2):
                        k = r % len(sides)
                        for label, fn, env in sides[k:] + sides[:k]:
                            ms = timed(fn, env)
                            if r >= 2:
                                t[label].append(ms)
                    if what == "miller":  # the last round left raw = general, ob = prepared Miller values: FExp both
                        _lib.check(lib.mlhip_final_exp_device(cid, raw.data_ptr(), n, oa.data_ptr(), st))
                        _lib.check(lib.mlhip_final_exp_device(cid, ob.data_ptr(), n, ob.data_ptr(), st))
                    torch.cuda.synchronize()
                    assert torch.equal(oa, ob), (name, what, ppp, n)
                    med = {k: statistics.median(v) for k, v in t.items()}
                    s = "%-9s %-7s ppp=%d n=%-6d" % (name, what, ppp, n)
                    for label, _, _ in sides:
                        s += "  %s %.3f [%.3f .. %.3f]" % (label, med[label], min(t[label]), max(t[label]))
                    s += "  ratio %.3f" % (med["general"] / med["prepared"])
                    emit(s)
        lib.mlhip_g2_prepared_destroy(h)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
