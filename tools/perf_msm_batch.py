#!/usr/bin/env python3
"""The batched MSM (mlhip_msm_batch*, mathlib_amd/csrc/msm_batch.h) over its grid: K in {2^10, 2^14, 2^16} segments x m in
{2, 4, 16, 64} pairs per segment plus one mixed-size batch, for BLS12-381 G1, BN254 G1 and BLS12-381 G2, every compiled
chunk length P (MLHIP_MSM_BATCH_CHUNK).  Per cell: the device form between device events after warm-up calls (median of
--reps), the host-buffer form by wall clock, and every output byte against cref.msm of its segment.  Beside them, on the
same box in the same run:
  (a) P = 1: one product per lane (what mlhip_scalar_mul on the same pairs plus a per-segment sum costs), and
      mlhip_scalar_mul_device alone on the same pairs ("scalar_mul" lines)
  (b) 256 separate mlhip_msm_g1 / _g2 host-buffer calls of the cell's first segments, the per-call floor ("single" lines)
  (c) cref.msm per segment on --threads host threads (ctypes drops the GIL), the CPU stand-in ("cref" lines)
One JSON line per cell on stdout and in --out.  Run on the GPU box: python tools/perf_msm_batch.py --out profiles/msm_batch_grid.jsonl
--grid small: K = 2^10 and 2^14 only (a quick look); --no-check: skip (c) and the byte checks."""
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
CHUNKS = (1, 2, 4, 8)
POOL = 1 << 16  # distinct points; pair i uses point i mod POOL (a segment of <= 64 pairs never holds a point twice)


def mixed_lengths(K: int, rng):
    """verifier-shaped: mostly 2 .. 8 pairs, some 16 .. 64, a few in the hundreds"""
    choice = rng.choice([2, 3, 4, 5, 7, 8, 16, 32, 64, 300], size=K, p=[0.2, 0.15, 0.15, 0.1, 0.1, 0.1, 0.08, 0.06, 0.05, 0.01])
    return [int(x) for x in choice]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--grid", choices=["full", "small"], default="full")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--configs", default="0,1,2", help="indices into CONFIGS")
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    out_f = open(args.out, "a") if args.out else None

    def emit(d):
        line = json.dumps(d, sort_keys=True)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    Ks = [1 << 10, 1 << 14] + ([1 << 16] if args.grid == "full" else [])
    ms = [2, 4, 16, 64]
    pool_ex = ThreadPoolExecutor(args.threads)
    for ci in [int(x) for x in args.configs.split(",")]:
        name, cid, group = CONFIGS[ci]
        _, g1b, g2b, _ = _lib.sizes(cid)
        ps = g1b if group == 1 else g2b
        pool = np.frombuffer(cref.gen_points(cid, group, 0x5EED, 0xC0DE, POOL), dtype=np.uint8).reshape(POOL, ps)
        d_pool = torch.from_numpy(pool.copy()).cuda()
        cells = [(K, m) for K in Ks for m in ms] + [(1 << 14, "mixed")]
        for K, m in cells:
            rng = np.random.default_rng(K * 131 + (m if m != "mixed" else 7))
            lengths = mixed_lengths(K, rng) if m == "mixed" else [m] * K
            offs = np.zeros(K + 1, dtype=np.uint64)
            offs[1:] = np.cumsum(lengths)
            n = int(offs[-1])
            idx = np.arange(n) % POOL
            scal = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
            scal[:, 3] |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)  # full 256-bit: most are >= r
            pts_h = pool[idx]  # (n, ps) host copy for the host form and cref
            d_pts = d_pool[torch.from_numpy(idx).cuda()].contiguous()
            d_sc = torch.from_numpy(scal.view(np.uint8).reshape(-1).copy()).cuda()
            d_out = torch.zeros(K * ps, dtype=torch.uint8, device="cuda")
            c_offs = offs.ctypes.data_as(ctypes.c_void_p)
            st = torch.cuda.current_stream()
            base = {"curve": name, "group": group, "K": K, "m": m, "pairs": n}

            # (c) cref per segment on host threads: the expected bytes
            ref, cref_s = None, None
            if not args.no_check:
                def seg(k):
                    a, b = int(offs[k]), int(offs[k + 1])
                    return cref.msm(cid, group, pts_h[a:b].tobytes(), scal[a:b].tobytes(), b - a, False, 0, 1)

                t = time.perf_counter()
                ref = b"".join(pool_ex.map(seg, range(K), chunksize=max(1, K // (4 * args.threads))))
                cref_s = time.perf_counter() - t
                emit(dict(base, kind="cref", threads=args.threads, ms=cref_s * 1e3, pairs_per_s=n / cref_s))

            for P in CHUNKS:
                os.environ["MLHIP_MSM_BATCH_CHUNK"] = str(P)

                def call():
                    _lib.check(lib.mlhip_msm_batch_device(cid, group, d_pts.data_ptr(), d_sc.data_ptr(), 0, c_offs, K,
                                                          d_out.data_ptr(), st.cuda_stream))

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
                dev_ms = statistics.median(times)
                got = d_out.cpu().numpy().tobytes()
                # host-buffer form
                pts_b, sc_b = pts_h.tobytes(), scal.tobytes()
                hout = ctypes.create_string_buffer(K * ps)
                _lib.check(lib.mlhip_msm_batch(cid, group, pts_b, sc_b, 0, c_offs, K, hout))
                ht = []
                for _ in range(max(2, args.reps // 2)):
                    t = time.perf_counter()
                    _lib.check(lib.mlhip_msm_batch(cid, group, pts_b, sc_b, 0, c_offs, K, hout))
                    ht.append(time.perf_counter() - t)
                host_ms = statistics.median(ht) * 1e3
                ok = None if ref is None else (got == ref and hout.raw == ref)
                emit(dict(base, kind="batch", P=P, device_ms=dev_ms, host_ms=host_ms, pairs_per_s=n / (dev_ms * 1e-3),
                          host_pairs_per_s=n / (host_ms * 1e-3), ok=ok))
                if ok is False:
                    bad = [k for k in range(K) if got[k * ps:(k + 1) * ps] != ref[k * ps:(k + 1) * ps]]
                    emit(dict(base, kind="mismatch", P=P, segments=bad[:20], count=len(bad)))
            os.environ.pop("MLHIP_MSM_BATCH_CHUNK", None)

            # (a) the per-pair products alone (mlhip_scalar_mul_device, double-and-add kernel)
            d_prod = torch.zeros(n * ps, dtype=torch.uint8, device="cuda")

            def smul():
                _lib.check(lib.mlhip_scalar_mul_device(cid, group, d_pts.data_ptr(), 1, d_sc.data_ptr(), 0, n, d_prod.data_ptr(),
                                                       st.cuda_stream))

            smul()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                smul()
                e1.record(st)
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            sm = statistics.median(times)
            emit(dict(base, kind="scalar_mul", device_ms=sm, pairs_per_s=n / (sm * 1e-3)))
            del d_prod

            # (b) separate single-MSM calls of the first 256 segments, host buffers (what the Go shim's MultiScalarMul does)
            fn = lib.mlhip_msm_g1 if group == 1 else lib.mlhip_msm_g2
            o1 = ctypes.create_string_buffer(ps)
            segs = [(int(offs[k]), int(offs[k + 1])) for k in range(min(256, K))]
            bufs = [(pts_h[a:b].tobytes(), scal[a:b].tobytes(), b - a) for a, b in segs]
            _lib.check(fn(cid, bufs[0][0], bufs[0][1], 0, bufs[0][2], 0, o1))
            t = time.perf_counter()
            for p_, s_, c_ in bufs:
                _lib.check(fn(cid, p_, s_, 0, c_, 0, o1))
            single_s = time.perf_counter() - t
            sp = sum(c for _, _, c in bufs)
            emit(dict(base, kind="single", calls=len(bufs), ms_per_call=single_s * 1e3 / len(bufs), pairs_per_s=sp / single_s))
            del d_pts, d_sc, d_out
            torch.cuda.empty_cache()
        del d_pool
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
