#!/usr/bin/env python3
"""K Miller-loop products of m > 4 pairs in one call (include/mlhip.h: "products of any length") measured on one GPU; prints
the text kept as profiles/miller_products_ab.txt.

  --sweep          the long call with MLHIP_MILLER_GROUP forced to 1, 2 and 4 (and the library's own pick) over the grid of
                   --ab: what miller_group_pick (pairing_products.h) is read from
                   (--big: 2^17 and 2^18 pairs instead, around the switch of the group size)
  --ab             the long call against what a caller could do before it, in one process, interleaved: on inputs transposed
                   slot-major BEFOREHAND (not timed), ceil(m / 4) mlhip_miller_loop_device calls at ppp = 4 and
                   ceil(m / 4) - 1 mlhip_gt_mul_device calls.  m in {8, 16, 64}, K from 1 to 2^16 / m on BLS12-381, two cells
                   on each of the other curves.  Both sides must give the same bytes.
  --parent-guard LIB   the kernels that gained arguments, from this tree's library and from LIB (the parent commit's build) as
                   alternating child processes: mlhip_miller_loop_device at ppp = 1 and 2 over 2^16 products,
                   mlhip_pairing_batch_device at 65 536, mlhip_pairing_prepared_device at ppp = 2; times, spread, output hashes

Inputs are seeded; a time is a host clock from the call to the end of a stream synchronisation, median of the rounds."""
import argparse
import hashlib
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

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
GRID_M = (8, 16, 64)


class Bench:
    def __init__(self):
        import torch

        from mathlib_amd import _lib

        self.torch, self._lib = torch, _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream()
        self.st = self.stream.cuda_stream
        self.cache = {}

    def points(self, name, n):
        """(curve id, n device G1 points, n device G2 points): seeded multiples of the generators, made once per curve"""
        if name not in self.cache or self.cache[name][3] < n:
            from conftest import load_golden

            torch, _lib = self.torch, self._lib
            g = load_golden(name)
            cid = g["curve_id"]
            _, g1b, g2b, _ = _lib.sizes(cid)
            gen = torch.Generator(device=self.dev)
            gen.manual_seed(23 + cid)
            out = []
            for group, size, key in ((1, g1b, "g1_gen"), (2, g2b, "g2_gen")):
                base = torch.frombuffer(bytearray(bytes.fromhex(g[key])), dtype=torch.uint8).to(self.dev)
                k = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, generator=gen, device=self.dev)
                k = k.view(torch.uint8).reshape(n, 32).contiguous()
                P = torch.empty(n * size, dtype=torch.uint8, device=self.dev)
                _lib.check(self.lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, k.data_ptr(), 0, n, P.data_ptr(), self.st))
                out.append(P)
            torch.cuda.synchronize()
            self.cache[name] = (cid, out[0], out[1], n)
        return self.cache[name][:3]

    def timed(self, fn):
        self.stream.synchronize()
        t0 = time.perf_counter()
        fn()
        self.stream.synchronize()
        return (time.perf_counter() - t0) * 1e3


def setenv(**kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def long_call(b, cid, P, Q, m, K, out):
    b._lib.check(b._lib.mlhip_miller_loop_products_device(b.lib, cid, P.data_ptr(), Q.data_ptr(), m, K, out.data_ptr(), b.st))


class Baseline:
    """the caller's own grouping: chunk j holds pairs 4 j .. 4 j + 3 of every product, contiguous (transposed beforehand)"""

    def __init__(self, b, cid, P, Q, m, K):
        torch = b.torch
        _, g1b, g2b, gtb = b._lib.sizes(cid)
        self.b, self.cid, self.K = b, cid, K
        p = P[: K * m * g1b].reshape(K, m, g1b)
        q = Q[: K * m * g2b].reshape(K, m, g2b)
        self.chunks = []
        for lo in range(0, m, 4):
            hi = min(m, lo + 4)
            self.chunks.append((hi - lo, p[:, lo:hi].contiguous(), q[:, lo:hi].contiguous()))
        self.part = [torch.empty(K * gtb, dtype=torch.uint8, device=b.dev) for _ in self.chunks]
        torch.cuda.synchronize()

    def run(self):
        b = self.b
        for (ppp, p, q), o in zip(self.chunks, self.part):
            b._lib.check(b.lib.mlhip_miller_loop_device(self.cid, p.data_ptr(), q.data_ptr(), ppp, self.K, o.data_ptr(), b.st))
        acc = self.part[0]
        for o in self.part[1:]:
            b._lib.check(b.lib.mlhip_gt_mul_device(self.cid, acc.data_ptr(), o.data_ptr(), self.K, acc.data_ptr(), b.st))
        return acc


def cells():
    for m in GRID_M:
        top = (1 << 16) // m
        for K in sorted({1, 64, 1024, top}):
            yield "BLS12-381", m, K
    for name in ("BN254", "BLS12-377"):
        yield name, 8, 64
        yield name, 16, 4096


def ab(b, out, rounds):
    out("== A/B: one long call (new) against ceil(m/4) mlhip_miller_loop_device calls at ppp = 4 + ceil(m/4) - 1 mlhip_gt_mul_device")
    out("   calls on slot-major inputs transposed beforehand (base), same process, %d interleaved rounds of new / base / base again" % rounds)
    out("   (all six orders in turn); ms = median; spread = |base - base again| / base; verdict: slower only beyond the spread")
    worst = 0
    for name, m, K in cells():
        cid, P, Q = b.points(name, 1 << 16)
        gtb = b._lib.sizes(cid)[3]
        setenv(MLHIP_MILLER_GROUP=None)
        o_new = b.torch.empty(K * gtb, dtype=b.torch.uint8, device=b.dev)
        base = Baseline(b, cid, P, Q, m, K)
        fns = [lambda: long_call(b, cid, P, Q, m, K, o_new), base.run, base.run]
        for f in fns:
            for _ in range(2):
                b.timed(f)
        same = bool(b.torch.equal(o_new, base.run()))
        ts = [[], [], []]
        orders = list(itertools.permutations(range(3)))
        for r in range(rounds):
            for k in orders[r % 6]:
                ts[k].append(b.timed(fns[k]))
        t = [statistics.median(x) for x in ts]
        spread = abs(t[1] - t[2]) / t[1]
        ratio = t[0] / min(t[1], t[2])
        verdict = "ahead" if ratio < 1 - spread else "SLOWER" if ratio > 1 + spread else "tie"
        worst += verdict == "SLOWER"
        out("%-9s m=%2d K=%5d: new %8.3f ms | base %8.3f / %8.3f ms | new/base %.3f spread %.3f  %s  bytes %s" % (
            name, m, K, t[0], t[1], t[2], ratio, spread, verdict, "equal" if same else "DIFFERENT"))
    out("cells where the long call is slower than the baseline beyond its spread: %d" % worst)


def sweep(b, out, rounds, big):
    out("== sweep: the long call with per forced (MLHIP_MILLER_GROUP); ms, median of %d runs; * = what the library picks" % rounds)
    # --big: around the switch of the group size only (2^17 and 2^18 pairs), in place of the grid
    grid = [(name, 16, 1 << lg) for name in CURVES for lg in (13, 14)] if big else list(cells())
    for name, m, K in grid:
        cid, P, Q = b.points(name, max(1 << 16, m * K))
        gtb = b._lib.sizes(cid)[3]
        o = b.torch.empty(K * gtb, dtype=b.torch.uint8, device=b.dev)
        row = []
        for per in (None, "1", "2", "4"):
            setenv(MLHIP_MILLER_GROUP=per)
            f = lambda: long_call(b, cid, P, Q, m, K, o)
            b.timed(f)
            row.append(statistics.median(b.timed(f) for _ in range(rounds)))
        setenv(MLHIP_MILLER_GROUP=None)
        out("%-9s m=%2d K=%5d (%6d pairs): pick* %8.3f | per=1 %8.3f  per=2 %8.3f  per=4 %8.3f" % (
            (name, m, K, m * K) + tuple(row)))


def child():
    """one process of the parent guard: the four calls on whatever MLHIP_LIB names; prints one JSON line"""
    b = Bench()
    torch = b.torch
    n = 1 << 16
    cid, P, Q = b.points("BLS12-381", 2 * n)
    _, g1b, g2b, gtb = b._lib.sizes(cid)
    out = torch.empty(n * gtb, dtype=torch.uint8, device=b.dev)
    h = __import__("ctypes").c_void_p()
    qs = bytes(Q[: 2 * g2b].cpu().numpy().tobytes())
    b._lib.check(b.lib.mlhip_g2_prepared_create(cid, qs, 2, __import__("ctypes").byref(h)))
    calls = {
        "miller_ppp1": lambda: b.lib.mlhip_miller_loop_device(cid, P.data_ptr(), Q.data_ptr(), 1, n, out.data_ptr(), b.st),
        "miller_ppp2": lambda: b.lib.mlhip_miller_loop_device(cid, P.data_ptr(), Q.data_ptr(), 2, n, out.data_ptr(), b.st),
        "pairing_batch": lambda: b.lib.mlhip_pairing_batch_device(cid, P.data_ptr(), Q.data_ptr(), n, out.data_ptr(), b.st),
        "pairing_prepared_ppp2": lambda: b.lib.mlhip_pairing_prepared_device(h, P.data_ptr(), None, 2, n, out.data_ptr(), b.st),
    }
    res = {}
    for tag, fn in calls.items():
        call = lambda: b._lib.check(fn())
        for _ in range(2):
            b.timed(call)
        res[tag] = {"ms": statistics.median(b.timed(call) for _ in range(7)),
                    "sha": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}
    b.lib.mlhip_g2_prepared_destroy(h)
    print(json.dumps(res), flush=True)


def parent_guard(parent_lib, out):
    out("== parent guard: BLS12-381, 2^16 products; this tree's library against the parent commit's build (%s)," % os.path.basename(parent_lib))
    out("   alternating child processes, 3 each; ms = median of 7 calls per process; spread = (max - min) / median over a side's processes")
    libs = {"parent": parent_lib, "this": os.path.join(ROOT, "mathlib_amd", "libmlhip.so")}
    runs = {"parent": [], "this": []}
    for rep in range(3):
        for tag in ("parent", "this"):
            env = dict(os.environ, MLHIP_LIB=libs[tag])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=300, env=env)
            if r.returncode != 0:
                out("%s child failed (%d): %s" % (tag, r.returncode, r.stderr[-400:]))
                return 1
            runs[tag].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    bad = 0
    for call in runs["this"][0]:
        ms = {tag: [r[call]["ms"] for r in runs[tag]] for tag in runs}
        med = {tag: statistics.median(v) for tag, v in ms.items()}
        spread = max((max(v) - min(v)) / med[tag] for tag, v in ms.items())
        ratio = med["this"] / med["parent"]
        same = len({r[call]["sha"] for tag in runs for r in runs[tag]}) == 1
        verdict = "within the spread" if abs(ratio - 1) <= spread else ("ahead" if ratio < 1 else "SLOWER")
        bad += verdict == "SLOWER" or not same
        out("%-22s parent %s | this %s | this/parent %.4f spread %.4f  %s  outputs %s" % (
            call, " ".join("%.3f" % v for v in ms["parent"]), " ".join("%.3f" % v for v in ms["this"]), ratio, spread, verdict,
            "identical" if same else "DIFFERENT"))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--big", action="store_true", help="--sweep: 2^17 and 2^18 pairs, around the switch of the group size, in place of the grid")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--rounds", type=int, default=12, help="--ab: interleaved rounds (a multiple of 6); --sweep: runs per cell")
    ap.add_argument("--parent-guard", metavar="LIB", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also append the text to this file")
    args = ap.parse_args()
    if args.child:
        child()
        return 0
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
            sweep(b, out, args.rounds, args.big)
        if args.ab:
            ab(b, out, args.rounds)
    if args.parent_guard:
        rc = parent_guard(os.path.abspath(args.parent_guard), out)
    return rc


if __name__ == "__main__":
    sys.exit(main())
