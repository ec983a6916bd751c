#!/usr/bin/env python3
"""Best Pippenger window per problem size on this GPU (feeds pick_window in api_msm.hip): resident inputs, best of 3.
--bits B (anywhere on the command line): short-scalar plans (mlhip_msm_plan_create_bits) over scalars below 2^B -- feeds
pick_window_bits; widths that give the same effective (c', W) are listed once.  tools/perf_msm_bits.py --sweep adds phases."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_golden  # noqa: E402
from mathlib_amd import _lib  # noqa: E402

bits = 0
if "--bits" in sys.argv:
    k = sys.argv.index("--bits")
    bits = int(sys.argv[k + 1])
    del sys.argv[k : k + 2]
name = sys.argv[1] if len(sys.argv) > 1 else "BLS12-381"
group = int(sys.argv[2]) if len(sys.argv) > 2 else 1
step = int(sys.argv[3]) if len(sys.argv) > 3 else 2  # sizes 2^lg0, 2^(lg0 + step), ...
lg0 = int(sys.argv[4]) if len(sys.argv) > 4 else 4
lib = _lib.load()
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
gen = torch.Generator(device=dev)
gen.manual_seed(11)
g = load_golden(name)
cid = g["curve_id"]
fpb, g1b, g2b, gtb = _lib.sizes(cid)
sz = g1b if group == 1 else g2b


def rnd(k):
    return torch.randint(-(1 << 63), (1 << 63) - 1, (k, 4), dtype=torch.int64, generator=gen, device=dev).view(torch.uint8).reshape(k, 32).contiguous()


nmax = 1 << (22 if group == 1 else 20)
base = torch.frombuffer(bytearray(bytes.fromhex(g["g1_gen" if group == 1 else "g2_gen"])), dtype=torch.uint8).to(dev)
P = torch.empty(nmax * sz, dtype=torch.uint8, device=dev)
_lib.check(lib.mlhip_scalar_mul_device(cid, group, base.data_ptr(), 0, rnd(nmax).data_ptr(), 0, nmax, P.data_ptr(), st))
S = rnd(nmax)
if bits:  # every scalar below 2^bits
    limbs = S.view(torch.int64).reshape(nmax, 4)
    for limb in range(4):
        keep = min(64, max(0, bits - 64 * limb))
        if keep == 0:
            limbs[:, limb] = 0
        elif keep < 64:
            limbs[:, limb] &= (1 << keep) - 1
torch.cuda.synchronize()
lg = lg0
while (1 << lg) <= nmax:
    n = 1 << lg
    res = {}
    seen = set()
    for c in range(4, 21):
        if c > lg + 6:
            break
        try:
            plan = _lib.MsmPlan(cid, group, n, c, bits)
        except Exception:
            continue
        if bits and plan.window() in seen:  # the same effective (c', W) as a narrower request
            plan.close()
            continue
        seen.add(plan.window())
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            plan.run(P.data_ptr(), S.data_ptr(), n, False, st)
            best = min(best, time.perf_counter() - t0)
        plan.close()
        res[c] = best * 1e3
    bc = min(res, key=res.get)
    print("%s G%d%s n=2^%d: best c=%d (%.3f ms)  " % (name, group, " bits=%d" % bits if bits else "", lg, bc, res[bc]) + " ".join("c%d=%.3f" % (c, t) for c, t in sorted(res.items()) if t < 1.5 * res[bc]), flush=True)
    lg += step
