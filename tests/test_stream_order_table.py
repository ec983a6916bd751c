"""Every function include/mlhip.h exports with a `void* stream` parameter has a row in the table of
tests/stream_order_cases.py, which tests/test_stream_order_gpu.py runs on a busy stream; the table names nothing the header
does not export.  The list comes from the header itself (as in tests/test_api_coverage.py), so the next device form cannot
ship without a busy-stream test."""
import os
import re

from conftest import ROOT

import stream_order_cases as S


def _header():
    with open(os.path.join(ROOT, "include", "mlhip.h")) as f:
        return f.read()


def stream_entry_points(text):
    """the exported functions whose parameter list has a `void* stream`"""
    decls = re.findall(r"^MLHIP_API\b[^(;]*?\b(mlhip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    return sorted(name for name, params in decls if re.search(r"\bvoid\s*\*\s*stream\b", params))


def test_every_stream_entry_point_has_a_row():
    names = stream_entry_points(_header())
    assert len(names) >= 24 and "mlhip_msm_launch_shared" in names and "mlhip_gt_mul_device" in names, names
    rows = {r.entry for r in S.ROWS}
    assert not set(names) - rows, "takes a stream but has no busy-stream row: %s" % ", ".join(sorted(set(names) - rows))
    assert not rows - set(names), "in the table but not exported with a stream: %s" % ", ".join(sorted(rows - set(names)))


def test_rows_are_well_formed():
    text = " ".join(_header().split())
    ids = [r.id for r in S.ROWS]
    assert len(ids) == len(set(ids))
    for r in S.ROWS:
        # the sentence of the header the row cites for its ordering promise, and for being synchronous by contract
        assert r.promise in text, (r.id, r.promise)
        assert r.sync is None or r.sync in text, (r.id, r.sync)
    # the three curves serve about a third of the rows each
    per_curve = [sum(r.id.endswith("-" + name) for r in S.ROWS) for name in S.CURVES]
    assert sum(per_curve) == len(S.ROWS) and max(per_curve) - min(per_curve) <= 1, per_curve
    # synchronous by contract: mlhip_msm_run, mlhip_bases_msm_device and the prepared forms on the general kernels
    assert {r.entry for r in S.ROWS if r.sync} == {"mlhip_msm_run", "mlhip_bases_msm_device", "mlhip_miller_loop_prepared_device",
                                                   "mlhip_pairing_prepared_device"}
    # the host arrays (typed pointers; device memory travels as void*) of every entry point are scribbled on by some row
    decls = dict(re.findall(r"^MLHIP_API\b[^(;]*?\b(mlhip_\w+)\s*\(([^;]*?)\)\s*;", _header(), flags=re.M | re.S))
    for entry in {r.entry for r in S.ROWS}:
        in_header = set(re.findall(r"const\s+uint(?:32|64)_t\s*\*\s*(\w+)", decls[entry]))
        in_table = set().union(*(r.host_args for r in S.ROWS if r.entry == entry))
        assert in_header == in_table, (entry, in_header, in_table)
