#!/usr/bin/env python3
"""Device-result MSM plans (mlhip_msm_plan_create_device_result) measured against host-result plans on one GPU; prints the text
kept as profiles/msm_device_result_ab.txt.

  --ab             a host-result plan against a device-result plan, and against a second host-result plan (the A/B's own
                   spread), in one process, on the same device buffers, all at window_c = 0: BLS12-381 G1 at 2^16 and 2^20
                   points, BLS12-381 G2 at 2^18, BN254 G1 at 2^20, and a 2^20-base BLS12-381 G1 handle with shifted-base tables.
                   Per cell, interleaved single runs in alternating order, medians:
                     (a) call until the result is usable: host-result = the mlhip_msm_run call; device-result = run_device
                         followed by a stream synchronise (the result is then in device memory)
                     (b) 16 MSMs back to back on one plan and one stream: host-result = 16 runs; device-result = 16 runs into a
                         16-slot device array, one synchronise, one copy of the array to the host
                     (c) [5] of mlhip_msm_plan_timings: the host tail / the tail kernel
                   and whether the results are byte-equal.
  --parent-guard DIR   bench.py's default config from this tree and from the tree at DIR (the parent commit, built), as
                   alternating child processes (tools/perf_msm_bits.py: parent_guard)

Inputs are seeded; every plan is warmed up before it is timed."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from perf_msm_bits import Bench, parent_guard  # noqa: E402

ROUNDS = 24
BACK_TO_BACK = 16


class PlanRunner:
    """one plan of either flavour behind the same three calls"""

    def __init__(self, b, cid, group, n, device_result):
        self.b, self.n, self.device = b, n, device_result
        self.plan = b._lib.MsmPlan(cid, group, n, 0, device_result=device_result)
        self.psz = self.plan.point_bytes
        self.slots = b.torch.zeros(BACK_TO_BACK * self.psz, dtype=b.torch.uint8, device=b.dev)

    def one(self, P, S):
        """(a): the result usable -- in host memory (host-result) or in device memory (device-result)"""
        if not self.device:
            return self.plan.run(P.data_ptr(), S.data_ptr(), self.n, False, self.b.st)
        self.plan.run_device(P.data_ptr(), S.data_ptr(), self.n, False, self.b.st, self.slots.data_ptr())
        self.b.torch.cuda.current_stream().synchronize()
        return None

    def many(self, P, S):
        """(b): 16 results in host memory"""
        if not self.device:
            return [self.plan.run(P.data_ptr(), S.data_ptr(), self.n, False, self.b.st) for _ in range(BACK_TO_BACK)]
        for k in range(BACK_TO_BACK):
            self.plan.run_device(P.data_ptr(), S.data_ptr(), self.n, False, self.b.st, self.slots.data_ptr() + k * self.psz)
        self.b.torch.cuda.current_stream().synchronize()
        raw = bytes(self.slots.cpu().numpy().tobytes())
        return [raw[k * self.psz : (k + 1) * self.psz] for k in range(BACK_TO_BACK)]

    def result(self, P, S):
        return self.many(P, S)[BACK_TO_BACK - 1]

    def tail_ms(self, P, S):
        self.plan.set_profiling(True)
        self.one(P, S)
        t = self.plan.timings()["host_tail"]
        self.plan.set_profiling(False)
        return t

    def close(self):
        self.b.torch.cuda.synchronize()
        self.plan.close()


class HandleRunner:
    """the same over a mlhip_bases handle of either flavour (scalars in device memory)"""

    def __init__(self, b, cid, group, P, n, device_result):
        lib, _lib = b.lib, b._lib
        self.b, self.n, self.device = b, n, device_result
        self.psz = P.numel() // n
        self.h = ctypes.c_void_p()
        if device_result:
            _lib.check(_lib.mlhip_bases_create_device_result(lib, cid, group, P.data_ptr(), 1, n, 0, ctypes.byref(self.h)))
        else:
            _lib.check(lib.mlhip_bases_create_device(cid, group, P.data_ptr(), n, 0, ctypes.byref(self.h)))
        self.tables = _lib.plan_timings(lib, lib.mlhip_bases_plan(self.h))["tables"]
        self.slots = b.torch.zeros(BACK_TO_BACK * self.psz, dtype=b.torch.uint8, device=b.dev)

    def _host(self, S):
        out = ctypes.create_string_buffer(self.psz)
        self.b._lib.check(self.b.lib.mlhip_bases_msm_device(self.h, S.data_ptr(), 0, self.n, self.b.st, out))
        return out.raw

    def _dev(self, S, k):
        self.b._lib.check(self.b._lib.mlhip_bases_msm_to_device(self.b.lib, self.h, S.data_ptr(), 0, self.n, self.b.st,
                                                               self.slots.data_ptr() + k * self.psz))

    def one(self, P, S):
        if not self.device:
            return self._host(S)
        self._dev(S, 0)
        self.b.torch.cuda.current_stream().synchronize()
        return None

    def many(self, P, S):
        if not self.device:
            return [self._host(S) for _ in range(BACK_TO_BACK)]
        for k in range(BACK_TO_BACK):
            self._dev(S, k)
        self.b.torch.cuda.current_stream().synchronize()
        raw = bytes(self.slots.cpu().numpy().tobytes())
        return [raw[k * self.psz : (k + 1) * self.psz] for k in range(BACK_TO_BACK)]

    def result(self, P, S):
        return self.many(P, S)[BACK_TO_BACK - 1]

    def tail_ms(self, P, S):
        lib, _lib = self.b.lib, self.b._lib
        plan = lib.mlhip_bases_plan(self.h)
        _lib.check(lib.mlhip_msm_plan_set_profiling(plan, 1))
        self.one(P, S)
        t = _lib.plan_timings(lib, plan)["host_tail"]
        _lib.check(lib.mlhip_msm_plan_set_profiling(plan, 0))
        return t

    def close(self):
        self.b.torch.cuda.synchronize()
        self.b.lib.mlhip_bases_destroy(self.h)


def timed(fn, *args):
    t0 = time.perf_counter()
    fn(*args)
    return (time.perf_counter() - t0) * 1e3


def ab(b, out):
    out("== A/B: host-result plan (H) against device-result plan (D) and a second host-result plan (H2), window_c = 0, same device buffers")
    out("   %d interleaved rounds of one measurement per plan, the three plans in rotating order; medians, ms" % ROUNDS)
    out("   (a) call until the result is usable (H: mlhip_msm_run; D: run_device + stream synchronise)")
    out("   (b) %d MSMs back to back on one plan and one stream, results in host memory (H: %d runs; D: %d runs into a device array, one synchronise, one copy)" % ((BACK_TO_BACK,) * 3))
    out("   (c) [5] of mlhip_msm_plan_timings (H: host tail; D: tail kernel); spread = |H - H2| / H")
    cells = [("BLS12-381", 1, 16, False), ("BLS12-381", 1, 20, False), ("BLS12-381", 2, 18, False), ("BN254", 1, 20, False),
             ("BLS12-381", 1, 20, True)]
    for name, group, lg, handle in cells:
        n = 1 << lg
        cid, P, S = b.inputs(name, group, 1 << (20 if group == 1 else 18))
        sc = b.scalars(S, n, 252)
        Pn = P[: n * (P.numel() // (1 << (20 if group == 1 else 18)))]
        if handle:
            runners = [HandleRunner(b, cid, group, Pn, n, f) for f in (False, True, False)]
            label = "%-9s G%d n=2^%d handle (tables %d/%d/%d)" % ((name, group, lg) + tuple(int(r.tables) for r in runners))
        else:
            runners = [PlanRunner(b, cid, group, n, f) for f in (False, True, False)]
            label = "%-9s G%d n=2^%d plan c=%d W=%d" % ((name, group, lg) + runners[1].plan.window())
        try:
            res = [r.result(Pn, sc) for r in runners]
            for r in runners:
                for _ in range(3):
                    r.one(Pn, sc)
            ta, tb = [[], [], []], [[], [], []]
            for rnd in range(ROUNDS):
                order = [(rnd + k) % 3 for k in range(3)]
                if rnd % 2:
                    order.reverse()
                for k in order:
                    ta[k].append(timed(runners[k].one, Pn, sc))
                for k in order:
                    tb[k].append(timed(runners[k].many, Pn, sc))
            a = [statistics.median(t) for t in ta]
            m = [statistics.median(t) for t in tb]
            tails = [r.tail_ms(Pn, sc) for r in runners[:2]]
            out("%s: (a) H %.3f D %.3f H2 %.3f  D/H %.3f spread %.3f | (b) H %.3f D %.3f H2 %.3f  D/H %.3f spread %.3f | (c) H %.3f D %.3f | bytes %s" % (
                label, a[0], a[1], a[2], a[1] / min(a[0], a[2]), abs(a[0] - a[2]) / a[0], m[0], m[1], m[2], m[1] / min(m[0], m[2]),
                abs(m[0] - m[2]) / m[0], tails[0], tails[1], "equal" if len(set(res)) == 1 else "DIFFERENT"))
        finally:
            for r in runners:
                r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--parent-guard", metavar="DIR", default=None)
    ap.add_argument("--out", default=None, help="also append the text to this file (--ab alone: profiles/msm_device_result_ab.txt)")
    args = ap.parse_args()
    if args.ab and not args.out:
        args.out = os.path.join(ROOT, "profiles", "msm_device_result_ab.txt")
    sink = open(args.out, "a") if args.out else None

    def out(s):
        print(s, flush=True)
        if sink:
            sink.write(s + "\n")
            sink.flush()

    rc = 0
    if args.ab:
        b = Bench()
        out("# device: %s" % b.torch.cuda.get_device_name(0))
        ab(b, out)
    if args.parent_guard:
        rc = parent_guard(os.path.abspath(args.parent_guard), out, os.path.dirname(os.path.abspath(args.out)) if args.out else ROOT)
    return rc


if __name__ == "__main__":
    sys.exit(main())
