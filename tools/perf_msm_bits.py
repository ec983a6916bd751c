#!/usr/bin/env python3
"""Short-scalar MSM plans (mlhip_msm_plan_create_bits) measured on one GPU; prints the text kept as profiles/msm_bits_ab.txt.

  --sweep          BLS12-381 and BN254, G1, n = 2^16 and 2^20, 32 / 64 / 128-bit scalars, every window width from 10 to 20 the
                   plan accepts: step time and phase times (what pick_window_bits in api_msm.hip is read from)
  --ab             a short plan (window_c = 0) against a full-width plan (window_c = 0) and against a second full-width plan
                   (the A/B's own spread) on identical device buffers, interleaved, all scalars below 2^bits: G1 at 2^16 and
                   2^20 on the three curves, G2 at 2^18 on BLS12-381; 32 / 64 / 128 / fr_bits bits; then mlhip_msm_bits
                   against mlhip_msm_g1 from host memory at 2^20
  --parent-guard DIR   bench.py's default config from this tree and from the tree at DIR (the parent commit, built), as
                   alternating child processes: step time of both, their spread, and whether the dumped outputs are equal

Inputs are seeded; every plan is warmed up before it is timed; a time is a host clock around mlhip_msm_run, which returns
when the result is in host memory."""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FR_BITS = {"BN254": 254, "BLS12-381": 255, "BLS12-377": 253}


class Bench:
    def __init__(self):
        import torch

        from mathlib_amd import _lib

        self.torch, self._lib = torch, _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.cache = {}

    def inputs(self, name, group, n):
        """(curve id, device points, device 256-bit random rows) -- seeded, made once per (curve, group)"""
        key = (name, group)
        if key not in self.cache or self.cache[key][3] < n:
            from conftest import load_golden

            torch, _lib = self.torch, self._lib
            g = load_golden(name)
            cid = g["curve_id"]
            _, g1b, g2b, _ = _lib.sizes(cid)
            gen = torch.Generator(device=self.dev)
            gen.manual_seed(11 + cid + 16 * group)

            def rnd(k):
                return torch.randint(-(1 << 63), (1 << 63) - 1, (k, 4), dtype=torch.int64, generator=gen, device=self.dev)

            base = torch.frombuffer(bytearray(bytes.fromhex(g["g1_gen" if group == 1 else "g2_gen"])), dtype=torch.uint8).to(self.dev)
            P = torch.empty(n * (g1b if group == 1 else g2b), dtype=torch.uint8, device=self.dev)
            k = rnd(n).view(torch.uint8).reshape(n, 32).contiguous()
            _lib.check(self.lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, k.data_ptr(), 0, n, P.data_ptr(), self.st))
            S = rnd(n)
            torch.cuda.synchronize()
            self.cache[key] = (cid, P, S, n)
        return self.cache[key][:3]

    def scalars(self, S, n, bits):
        """the first n rows of S masked to `bits` bits, as device bytes"""
        torch = self.torch
        s = S[:n].clone()
        for limb in range(4):
            keep = min(64, max(0, bits - 64 * limb))
            if keep == 0:
                s[:, limb] = 0
            elif keep < 64:
                s[:, limb] &= (1 << keep) - 1
        return s.view(torch.uint8).reshape(n, 32).contiguous()

    def time_plan(self, plan, P, S, n, runs=3):
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            plan.run(P.data_ptr(), S.data_ptr(), n, False, self.st)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3


def sweep(b, out, sizes=(16, 20), g2=False):
    out("== sweep: step time (median of 9 runs after 3 warm-up runs, ms) and phases (digits / sort / accumulate / reduce / host tail, ms)")
    out("   per requested width c: the plan's effective width c' and window count W; scalars uniform below 2^bits")
    for name, group in [("BLS12-381", 1), ("BN254", 1)] + ([("BLS12-381", 2)] if g2 else []):
        for lg in sizes:
            if group == 2 and lg > 18:
                continue
            n = 1 << lg
            cid, P, S = b.inputs(name, group, 1 << max(max(sizes) if group == 1 else 18, 18))
            for bits in (32, 64, 128):
                sc = b.scalars(S, n, bits)
                rows, seen = [], set()
                for c in range(10, 21):
                    try:
                        plan = b._lib.MsmPlan(cid, group, n, c, bits)
                    except b._lib.MlhipError:
                        continue
                    geo = plan.window()
                    if geo in seen:  # another c with the same c' and W: the same plan
                        plan.close()
                        continue
                    seen.add(geo)
                    plan.run(P.data_ptr(), sc.data_ptr(), n, False, b.st)
                    slow = b.time_plan(plan, P, sc, n, 1)
                    if slow > 25.0:  # far from any optimum: one run is enough to say so
                        plan.close()
                        rows.append((slow, c, geo, None))
                        continue
                    plan.run(P.data_ptr(), sc.data_ptr(), n, False, b.st)
                    t = b.time_plan(plan, P, sc, n, 9)
                    plan.set_profiling(True)
                    plan.run(P.data_ptr(), sc.data_ptr(), n, False, b.st)
                    ph = plan.timings()
                    plan.close()
                    rows.append((t, c, geo, ph))
                pick = b._lib.MsmPlan(cid, group, n, 0, bits)
                picked = pick.window()
                pick.close()
                best = min(rows, key=lambda r: r[0])
                out("%s G%d n=2^%d bits=%d: library picks c'=%d W=%d; best c'=%d W=%d (%.3f ms)" % (name, group, lg, bits, picked[0], picked[1], best[2][0], best[2][1], best[0]))
                for t, c, geo, ph in rows:
                    out("    c=%2d c'=%2d W=%2d  %7.3f ms%s  %s" % (
                        c, geo[0], geo[1], t, " *" if geo == picked else "  ",
                        "phases %.3f / %.3f / %.3f / %.3f / %.3f" % (ph["digits"], ph["sort"], ph["accumulate"], ph["reduce"], ph["host_tail"]) if ph else "(one run)"))


def ab(b, out):
    out("== A/B: short plan (window_c = 0) against full-width plan (window_c = 0), same device buffers, scalars below 2^bits")
    out("   36 interleaved rounds of one run per plan (short, full, full again; all six orders in turn); time = median of a plan's 36 runs, ms")
    out("   spread = |full - full again| / full: what two runs of the SAME plan differ by; predicted = W_short / W_full (additions)")
    cells = [(name, 1, lg) for name in ("BLS12-381", "BN254", "BLS12-377") for lg in (16, 20)] + [("BLS12-381", 2, 18)]
    for name, group, lg in cells:
        n = 1 << lg
        cid, P, S = b.inputs(name, group, 1 << (20 if group == 1 else 18))
        for bits in (32, 64, 128, FR_BITS[name]):
            sc = b.scalars(S, n, min(bits, 252))  # (full width: below every r, so that no plan reduces anything)
            full = b._lib.MsmPlan(cid, group, n, 0)  # (created first, the short plan between the two full-width ones)
            plans = [b._lib.MsmPlan(cid, group, n, 0, bits), full, b._lib.MsmPlan(cid, group, n, 0)]
            res = [p.run(P.data_ptr(), sc.data_ptr(), n, False, b.st) for p in plans]
            for p in plans:
                for _ in range(3):
                    p.run(P.data_ptr(), sc.data_ptr(), n, False, b.st)
            rounds = [[], [], []]
            orders = list(itertools.permutations(range(3)))
            for r in range(36):  # single runs, every order of the three plans in turn: no plan always follows the same one
                for k in orders[r % 6]:
                    rounds[k].append(b.time_plan(plans[k], P, sc, n, 1))
            t = [statistics.median(r) for r in rounds]
            geo = [p.window() for p in plans]
            for p in plans:
                p.close()
            spread = abs(t[1] - t[2]) / t[1]
            ratio = t[0] / min(t[1], t[2])
            verdict = "same plan" if bits == FR_BITS[name] else ("ahead" if ratio < 1 - spread else "slower" if ratio > 1 + spread else "tie")
            out("%-9s G%d n=2^%d bits=%3d: short c'=%2d W=%2d %7.3f ms | full c=%2d W=%2d %7.3f / %7.3f ms | short/full %.3f (predicted %.3f) spread %.3f  %s  bytes %s" % (
                name, group, lg, bits, geo[0][0], geo[0][1], t[0], geo[1][0], geo[1][1], t[1], t[2], ratio, geo[0][1] / geo[1][1], spread, verdict,
                "equal" if len(set(res)) == 1 else "DIFFERENT"))
    out("== host memory, BLS12-381 G1 n=2^20: mlhip_msm_bits against mlhip_msm_g1 (window_c = 0), 8 interleaved calls each, median, ms")
    import ctypes

    cid, P, S = b.inputs("BLS12-381", 1, 1 << 20)
    n = 1 << 20
    hp = bytes(P.cpu().numpy().tobytes())
    o1, o2 = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    for bits in (32, 64, 128, 255):
        hs = bytes(b.scalars(S, n, min(bits, 252)).cpu().numpy().tobytes())
        ta, tb = [], []
        for i in range(10):
            t0 = time.perf_counter()
            b._lib.check(b._lib.mlhip_msm_bits(b.lib, cid, 1, hp, hs, 0, bits, n, 0, o1))
            t1 = time.perf_counter()
            b._lib.check(b.lib.mlhip_msm_g1(cid, hp, hs, 0, n, 0, o2))
            t2 = time.perf_counter()
            if i >= 2:  # the first two calls create the pooled plans
                ta.append((t1 - t0) * 1e3)
                tb.append((t2 - t1) * 1e3)
        out("bits=%3d: mlhip_msm_bits %7.3f ms | mlhip_msm_g1 %7.3f ms | ratio %.3f  bytes %s" % (
            bits, statistics.median(ta), statistics.median(tb), statistics.median(ta) / statistics.median(tb), "equal" if o1.raw == o2.raw else "DIFFERENT"))


def parent_guard(parent_dir, out, work):
    import numpy as np

    out("== parent guard: bench.py --gpus 1 --steps 30 --warmup 5 (default config), this tree against the parent commit's build,")
    out("   alternating child processes, 3 each; ms per step")
    ms = {"parent": [], "this": []}
    dumps = {}
    for rep in range(3):
        for tag, root in (("parent", parent_dir), ("this", ROOT)):
            dump = os.path.join(work, "dump_%s" % tag)
            cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5", "--no-cpu-baseline",
                   "--no-pairing", "--no-extras", "--dump-outputs", dump]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root)
            if r.returncode != 0:
                out("%s bench.py failed (%d): %s" % (tag, r.returncode, r.stderr[-400:]))
                return 1
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            ms[tag].append(line["ms_per_step"])
            dumps[tag] = {f: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump)) if f.endswith(".npy")}
    same = dumps["parent"].keys() == dumps["this"].keys() and all(np.array_equal(dumps["parent"][k], dumps["this"][k]) for k in dumps["this"])
    for tag in ("parent", "this"):
        out("%-6s %s  median %.4f  spread (max - min) / median %.4f" % (tag, " ".join("%.4f" % v for v in ms[tag]), statistics.median(ms[tag]),
                                                                      (max(ms[tag]) - min(ms[tag])) / statistics.median(ms[tag])))
    out("this / parent = %.4f ; dumped outputs %s" % (statistics.median(ms["this"]) / statistics.median(ms["parent"]), "identical" if same else "DIFFERENT"))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--sizes", default="16,20", help="--sweep: log2 of the sizes (default 16,20)")
    ap.add_argument("--g2", action="store_true", help="--sweep: BLS12-381 G2 as well (sizes up to 2^18)")
    ap.add_argument("--parent-guard", metavar="DIR", default=None)
    ap.add_argument("--out", default=None, help="also append the text to this file")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def out(s):
        print(s, flush=True)
        if sink:
            sink.write(s + "\n")
            sink.flush()

    rc = 0
    if args.sweep or args.ab:
        b = Bench()
        out("# device: %s" % b.torch.cuda.get_device_name(0))
        if args.sweep:
            sweep(b, out, tuple(int(v) for v in args.sizes.split(",")), args.g2)
        if args.ab:
            ab(b, out)
    if args.parent_guard:
        rc = parent_guard(os.path.abspath(args.parent_guard), out, os.path.dirname(os.path.abspath(args.out)) if args.out else ROOT)
    return rc


if __name__ == "__main__":
    sys.exit(main())
