#!/usr/bin/env python3
"""Shared-scalar MSMs over a set of resident-bases handles (mlhip_bases_set_create) measured against the members' own calls on
one GPU; prints the text kept as profiles/bases_set_ab.txt.

  --ab             per cell, in one process on the same handles and the same scalar buffer:
                     set   one mlhip_bases_msm[_device] call on the set, shared route (MLHIP_BASES_SET_SHARE=1)
                     sep   k mlhip_bases_msm[_device] calls, one per member
                     sep'  the k calls again, into outputs of their own: the A/B's own spread
                   Interleaved single runs in rotating order, 2 warm-up rounds, medians of 7 rounds; the outputs of the three
                   sides are compared byte for byte.  Grid: BLS12-381 and BN254; members {G1, G2} at 2^12, 2^16, 2^20, 2^22 and
                   {G1, G1, G2} at 2^12, 2^16, 2^20; host scalars and device scalars; shifted-base tables on
                   (MLHIP_BASES_TABLES=1, the library's digit width and tile for the size).
  --sizes a,b,..   log2 of the sizes instead (a size above 2^20 runs {G1, G2} only)
  --parent-guard DIR   bench.py's default config from this tree and from the tree at DIR (the parent commit, built), as
                   alternating child processes (tools/perf_msm_bits.py: parent_guard)

Inputs are seeded; every handle has run once before it is timed."""
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

WARMUP, ROUNDS = 2, 7


def cell(b, out, name, groups, lg, device_scalars):
    torch, _lib, lib = b.torch, b._lib, b.lib
    n = 1 << lg
    handles, psz = [], []
    S = None
    os.environ["MLHIP_BASES_TABLES"] = "1"
    try:
        for i, g in enumerate(groups):
            cid, P, S = b.inputs(name, g, n)
            sz = _lib.sizes(cid)[g]
            rows = P[: n * sz].reshape(n, sz)
            if i and g in groups[:i]:  # a second table of the same group: the same points in another order
                rows = torch.roll(rows, 1 + i, 0).contiguous()
            h = ctypes.c_void_p()
            _lib.check(lib.mlhip_bases_create_device(cid, g, rows.data_ptr(), n, 0, ctypes.byref(h)))
            handles.append(h)
            psz.append(sz)
        s = _lib.bases_set_create(lib, handles)
    finally:
        del os.environ["MLHIP_BASES_TABLES"]
    d_sc = S[:n].view(torch.uint8).reshape(n, 32).contiguous()
    h_sc = bytes(d_sc.cpu().numpy().tobytes())
    torch.cuda.synchronize()
    total = sum(psz)
    outs = {tag: ctypes.create_string_buffer(total) for tag in ("set", "sep", "sep'")}
    offs = [sum(psz[:i]) for i in range(len(psz))]

    def run_set(buf):
        if device_scalars:
            _lib.check(lib.mlhip_bases_msm_device(s, d_sc.data_ptr(), 0, n, b.st, buf))
        else:
            _lib.check(lib.mlhip_bases_msm(s, h_sc, 0, n, buf))

    def run_sep(buf):
        for h, off in zip(handles, offs):
            dst = ctypes.byref(buf, off)
            if device_scalars:
                _lib.check(lib.mlhip_bases_msm_device(h, d_sc.data_ptr(), 0, n, b.st, dst))
            else:
                _lib.check(lib.mlhip_bases_msm(h, h_sc, 0, n, dst))

    sides = [("set", run_set), ("sep", run_sep), ("sep'", run_sep)]
    ms = {tag: [] for tag, _ in sides}
    os.environ["MLHIP_BASES_SET_SHARE"] = "1"
    try:
        for r in range(WARMUP + ROUNDS):
            for j in range(3):
                tag, fn = sides[(r + j) % 3]
                t0 = time.perf_counter()
                fn(outs[tag])
                dt = 1e3 * (time.perf_counter() - t0)
                if r >= WARMUP:
                    ms[tag].append(dt)
        route = _lib.bases_set_route(lib, s)
    finally:
        del os.environ["MLHIP_BASES_SET_SHARE"]
    same = outs["set"].raw == outs["sep"].raw == outs["sep'"].raw
    med = {tag: statistics.median(v) for tag, v in ms.items()}
    spread = abs(med["sep"] - med["sep'"]) / min(med["sep"], med["sep'"])
    sep = min(med["sep"], med["sep'"])
    ratio = med["set"] / sep
    tables = [_lib.plan_timings(lib, lib.mlhip_bases_plan(h)) for h in handles]
    geo = "/".join("c%d%s" % (int(t["window_c"]), "t" if t.get("tables") == 1.0 else "p") for t in tables)
    out("%-9s %-8s 2^%-2d %-6s  set %8.3f  sep %8.3f  sep' %8.3f ms  set/sep %.3f  spread %.3f  %s  route %s  %s  %s" % (
        name, "+".join("G%d" % g for g in groups), lg, "device" if device_scalars else "host", med["set"], med["sep"], med["sep'"], ratio,
        spread, "SLOWER" if ratio > 1 + spread else "ok", route, geo, "bytes equal" if same else "BYTES DIFFER"))
    lib.mlhip_bases_destroy(s)
    for h in handles:
        lib.mlhip_bases_destroy(h)
    torch.cuda.synchronize()
    return same


def ab(b, out, sizes):
    out("== set call (shared route) against k separate handle calls on the same buffers; medians of %d rounds after %d warm-up rounds," % (ROUNDS, WARMUP))
    out("   interleaved in rotating order; spread = |sep - sep'| / min; geometry: c<digit width><t = tables, p = plain> per member")
    ok = True
    for name in ("BLS12-381", "BN254"):
        for groups in ((1, 2), (1, 1, 2)):
            for lg in sizes:
                if lg > 20 and len(groups) > 2:
                    continue
                for device_scalars in (False, True):
                    ok = cell(b, out, name, groups, lg, device_scalars) and ok
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--sizes", default="12,16,20,22")
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
    if args.ab:
        b = Bench()
        out("# device: %s" % b.torch.cuda.get_device_name(0))
        rc = ab(b, out, tuple(int(v) for v in args.sizes.split(",")))
    if args.parent_guard:
        rc = parent_guard(os.path.abspath(args.parent_guard), out, os.path.dirname(os.path.abspath(args.out)) if args.out else ROOT) or rc
    return rc


if __name__ == "__main__":
    sys.exit(main())
