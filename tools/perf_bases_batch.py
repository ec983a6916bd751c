#!/usr/bin/env python3
"""The batched MSM over resident bases (mlhip_bases_msm_batch*, mathlib_amd/csrc/msm_bases_batch.h) over its grid: L = 64
bases of one handle, K in {2^10, 2^14, 2^16} segments x m in {2, 4, 16, 64} pairs per segment, with an index list (random
bases) and without (pair j of a segment takes base j), for BLS12-381 G1, BN254 G1 and BLS12-381 G2.  Per cell, on the same
pairs, the device form between device events after two warm-up calls (median of --reps) of
  (a) the table path (the defaults: per-base fixed-window tables),
  (b) MLHIP_BASES_BATCH_MAX_MB=0 (the table-free path: mlhip_msm_batch's body over the handle's points), and
  (c) mlhip_msm_batch_device on the materialised points (the caller gathers them),
and every output byte of all three against cref.msm of its segment (on --threads host threads).  Besides the grid:
  "build" lines   the table build time (first call minus a warm call, wall clock) and the table bytes for every width swept
  "sweep" lines   width w x chunk length P on the verifier-sized cells (2^14 and 2^16 segments of 4 and 16 pairs)
One JSON line per measurement on stdout and in --out.  Run on the GPU box:
  python tools/perf_bases_batch.py --out profiles/bases_batch_grid.jsonl
--parts picks among grid, build, sweep; --grid small: K = 2^10 and 2^14 only; --no-check: skip cref (outputs of (a), (b)
and (c) are still compared with each other)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mathlib_amd import _lib  # noqa: E402
from oracle import cref  # noqa: E402

CONFIGS = [("BLS12-381", 1, 1), ("BN254", 0, 1), ("BLS12-381", 1, 2)]
L_BASES = 64
WIDTHS = (4, 5, 6, 7, 8, 10, 12)
CHUNKS = (1, 2, 4, 8, 16)
ENV = ("MLHIP_BASES_BATCH_WINDOW", "MLHIP_BASES_BATCH_CHUNK", "MLHIP_BASES_BATCH_MAX_MB")


def set_env(**kv):
    for k in ENV:
        os.environ.pop(k, None)
    for k, v in kv.items():
        os.environ["MLHIP_BASES_BATCH_" + k] = str(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--grid", choices=["full", "small"], default="full")
    ap.add_argument("--parts", default="build,sweep,grid")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--configs", default="0,1,2", help="indices into CONFIGS")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    import torch

    lib = _lib.load()
    out_f = open(args.out, "a") if args.out else None
    pool_ex = ThreadPoolExecutor(args.threads)
    st = torch.cuda.current_stream()

    def emit(d):
        line = json.dumps(d, sort_keys=True)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    def timed(call):
        call()
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    for ci in [int(x) for x in args.configs.split(",")]:
        name, cid, group = CONFIGS[ci]
        _, g1b, g2b, _ = _lib.sizes(cid)
        ps = g1b if group == 1 else g2b
        fp_bytes = g1b // 2
        row = (2 if group == 1 else 4) * (56 if fp_bytes == 48 else 40)  # Affine28 / AffineG2_28 bytes
        bases_b = cref.gen_points(cid, group, 0xBA5E, 0x64, L_BASES)
        bases = np.frombuffer(bases_b, dtype=np.uint8).reshape(L_BASES, ps)
        d_bases = torch.from_numpy(bases.copy()).cuda()

        def new_handle():
            h = ctypes.c_void_p()
            _lib.check(lib.mlhip_bases_create(cid, group, bases_b, L_BASES, 0, ctypes.byref(h)))
            return h

        def tabled(h):
            n = ctypes.c_size_t()
            _lib.check(lib.mlhip_bases_batch_tabled(h, ctypes.byref(n)))
            return n.value

        def cell_data(K, m, indexed, seed):
            rng = np.random.default_rng(seed)
            offs = np.zeros(K + 1, dtype=np.uint64)
            offs[1:] = np.arange(1, K + 1, dtype=np.uint64) * np.uint64(m)
            n = K * m
            idx = (rng.integers(0, L_BASES, size=n) if indexed else np.tile(np.arange(m), K)).astype(np.uint32)
            scal = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
            scal[:, 3] |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)  # full 256-bit: most are >= r
            return offs, idx, scal

        def reference(offs, idx, scal):
            if args.no_check:
                return None, None
            K = len(offs) - 1
            pts_h = bases[idx]

            def seg(k):
                a, b = int(offs[k]), int(offs[k + 1])
                return cref.msm(cid, group, pts_h[a:b].tobytes(), scal[a:b].tobytes(), b - a, False, 0, 1)

            t = time.perf_counter()
            ref = b"".join(pool_ex.map(seg, range(K), chunksize=max(1, K // (4 * args.threads))))
            return ref, time.perf_counter() - t

        def runner(h, offs, idx, scal, indexed):
            K = len(offs) - 1
            d_sc = torch.from_numpy(scal.view(np.uint8).reshape(-1).copy()).cuda()
            d_out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
            c_offs = offs.ctypes.data_as(ctypes.c_void_p)
            c_idx = idx.ctypes.data_as(ctypes.c_void_p) if indexed else None

            def call():
                _lib.check(lib.mlhip_bases_msm_batch_device(h, d_sc.data_ptr(), 0, c_idx, c_offs, K, st.cuda_stream, d_out.data_ptr()))

            return call, d_out, d_sc

        if "build" in parts:
            for w in WIDTHS:
                set_env(WINDOW=w, MAX_MB=1 << 16)
                h = new_handle()
                offs, idx, scal = cell_data(1, L_BASES, False, 1)
                call, d_out, _ = runner(h, offs, idx, scal, False)
                torch.cuda.synchronize()
                t = time.perf_counter()
                call()
                torch.cuda.synchronize()
                first = time.perf_counter() - t
                t = time.perf_counter()
                call()
                torch.cuda.synchronize()
                warm = time.perf_counter() - t
                ref, _ = reference(offs, idx, scal)
                ok = None if ref is None else d_out.cpu().numpy().tobytes() == ref
                entries = -(-256 // w) << (w - 1)
                emit(dict(kind="build", curve=name, group=group, w=w, bases=L_BASES, tabled=tabled(h), build_ms=(first - warm) * 1e3,
                          table_bytes=L_BASES * entries * row, bytes_per_base=entries * row, ok=ok))
                lib.mlhip_bases_destroy(h)

        if "sweep" in parts:
            h = new_handle()
            for K in (1 << 14, 1 << 16):
                for m in (4, 16):
                    offs, idx, scal = cell_data(K, m, True, K * 7 + m)
                    ref, _ = reference(offs, idx, scal)
                    for w in WIDTHS:
                        for P in CHUNKS:
                            set_env(WINDOW=w, CHUNK=P, MAX_MB=1 << 16)
                            call, d_out, _ = runner(h, offs, idx, scal, True)
                            ms = timed(call)
                            got = d_out.cpu().numpy().tobytes()
                            emit(dict(kind="sweep", curve=name, group=group, K=K, m=m, w=w, P=P, device_ms=ms,
                                      pairs_per_s=K * m / (ms * 1e-3), ok=None if ref is None else got == ref))
            lib.mlhip_bases_destroy(h)

        if "grid" in parts:
            Ks = [1 << 10, 1 << 14] + ([1 << 16] if args.grid == "full" else [])
            h = new_handle()
            for K in Ks:
                for m in (2, 4, 16, 64):
                    for indexed in (True, False):
                        offs, idx, scal = cell_data(K, m, indexed, K * 13 + m + indexed)
                        ref, cref_s = reference(offs, idx, scal)
                        base = dict(curve=name, group=group, K=K, m=m, pairs=K * m, indexed=indexed, bases=L_BASES)
                        res = {}
                        for col, env in (("a", {}), ("b", {"MAX_MB": 0})):
                            set_env(**env)
                            call, d_out, _ = runner(h, offs, idx, scal, indexed)
                            res[col] = (timed(call), d_out.cpu().numpy().tobytes(), tabled(h))
                        set_env()
                        d_pts = d_bases[torch.from_numpy(idx.astype(np.int64)).cuda()].contiguous()
                        d_sc = torch.from_numpy(scal.view(np.uint8).reshape(-1).copy()).cuda()
                        d_out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
                        c_offs = offs.ctypes.data_as(ctypes.c_void_p)

                        def call_c():
                            _lib.check(lib.mlhip_msm_batch_device(cid, group, d_pts.data_ptr(), d_sc.data_ptr(), 0, c_offs, K,
                                                                  d_out.data_ptr(), st.cuda_stream))

                        res["c"] = (timed(call_c), d_out.cpu().numpy().tobytes(), None)
                        same = res["a"][1] == res["b"][1] == res["c"][1]
                        ok = same if ref is None else same and res["a"][1] == ref
                        emit(dict(base, kind="cell", a_ms=res["a"][0], b_ms=res["b"][0], c_ms=res["c"][0],
                                  a_pairs_per_s=K * m / (res["a"][0] * 1e-3), a_over_c=res["c"][0] / res["a"][0],
                                  b_over_c=res["c"][0] / res["b"][0], tabled_a=res["a"][2], tabled_b=res["b"][2],
                                  cref_ms=None if cref_s is None else cref_s * 1e3, ok=ok))
                        del d_pts, d_sc, d_out
            lib.mlhip_bases_destroy(h)
            torch.cuda.empty_cache()
        del d_bases
    set_env()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
