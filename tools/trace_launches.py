#!/usr/bin/env python3
"""Do two builds launch the same kernels?  Reduces rocprofv3 kernel traces (every *kernel_trace.csv below a directory) to
the multiset of (kernel name, grid, workgroup, LDS bytes) and, where the trace names the queue, to the ordered list of
those launches per queue (queues numbered in order of first use), and compares two such reductions.  The HIP runtime's own
copy and fill kernels (__amd_rocclr_*: how it chooses to carry out a hipMemcpy / hipMemset, per call and per run) are
counted and compared apart from the library's launches and do not enter the verdict.

Usage: trace_launches.py <dir A> [<dir B>]   -- one directory: its counts per kernel; two: the counts and "equal" or the
differences; exit status 1 when they differ."""
import collections
import csv
import os
import sys


def column(fields, *prefixes):
    return [f for f in fields if any(f.lower().startswith(p) for p in prefixes)]


def reduce_dir(root):
    launches, runtime = collections.Counter(), collections.Counter()
    queues = []  # per trace file and queue, in order of first use: the ordered launches
    for d, _, files in sorted(os.walk(root)):
        for name in sorted(files):
            if not name.endswith("kernel_trace.csv"):
                continue
            with open(os.path.join(d, name), newline="") as f:
                rows = list(csv.DictReader(f))
            if not rows:
                continue
            fields = list(rows[0])
            grid, wg = column(fields, "grid_size"), column(fields, "workgroup_size")
            lds = column(fields, "lds_block_size", "group_segment_size")
            queue = column(fields, "queue_id")
            order = column(fields, "dispatch_id") or column(fields, "start_timestamp")
            rows.sort(key=lambda r: int(r[order[0]]))
            per_queue = collections.OrderedDict()
            for r in rows:
                k = (r["Kernel_Name"], tuple(int(r[c]) for c in grid), tuple(int(r[c]) for c in wg), tuple(int(r[c]) for c in lds))
                if k[0].startswith("__amd_rocclr_"):
                    runtime[k] += 1
                    continue
                launches[k] += 1
                if queue:
                    per_queue.setdefault(r[queue[0]], []).append(k)
            queues += list(per_queue.values())
    return launches, queues, runtime


def short(name):
    return name.split("(")[0].replace("void ", "").replace("mlhip::", "")


def main(argv):
    a, qa, ra = reduce_dir(argv[1])
    per_kernel = collections.Counter()
    for k, c in a.items():
        per_kernel[short(k[0])] += c
    print("# %d launches of %d kernels in %d shapes (name, grid, workgroup, LDS), %d queues" % (sum(a.values()), len(per_kernel), len(a), len(qa)))
    for k in sorted(per_kernel):
        print("%-60s %8d" % (k, per_kernel[k]))
    for k in sorted(set(short(k[0]) for k in ra)):
        print("%-60s %8d   (runtime)" % (k, sum(c for q, c in ra.items() if short(q[0]) == k)))
    if len(argv) < 3:
        return 0
    b, qb, rb = reduce_dir(argv[2])
    rc = 0
    if a == b:
        print("multiset of (kernel, grid, workgroup, LDS): equal (%d launches)" % sum(b.values()))
    else:
        rc = 1
        print("multiset of (kernel, grid, workgroup, LDS): DIFFERS")
        for k in sorted(set(a) | set(b)):
            if a[k] != b[k]:
                print("  %s grid=%s wg=%s lds=%s: %d against %d" % (short(k[0]), k[1], k[2], k[3], a[k], b[k]))
    if ra == rb:
        print("runtime copy / fill kernels: equal (%d launches)" % sum(rb.values()))
    else:
        for k in sorted(set(ra) | set(rb)):
            if ra[k] != rb[k]:
                print("runtime copy / fill kernels: %s grid=%s wg=%s: %d against %d" % (short(k[0]), k[1], k[2], ra[k], rb[k]))
    if qa or qb:
        if qa == qb:
            print("ordered launches per queue: equal (%d queues)" % len(qa))
        else:
            rc = 1
            print("ordered launches per queue: DIFFER (%d against %d queues)" % (len(qa), len(qb)))
            for i, (x, y) in enumerate(zip(qa, qb)):
                if x != y:
                    j = next((j for j, (u, v) in enumerate(zip(x, y)) if u != v), min(len(x), len(y)))
                    print("  queue %d: %d against %d launches, first difference at launch %d: %s against %s" % (
                        i, len(x), len(y), j, short(x[j][0]) if j < len(x) else None, short(y[j][0]) if j < len(y) else None))
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv))
