"""The model of tests/msm_geometry_cases.py, checked on the CPU: its digit replica against the kernels' own digit body
(hm_digits of the host-math library), its constants against the headers, and every fact a case claims -- which bin goes to
which fine-sort path with which slices, which bucket is long, what the launch makes of a tile request -- against the model.
tests/test_msm_geometry_gpu.py runs the same cases on the GPU; this file is what shows that they reach their branches.

The case table (python tests/test_msm_geometry_host.py prints it): one line per run of a case with the facts asserted."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT  # (puts the repository root on sys.path: the cases import the oracle)

import msm_geometry_cases as G  # noqa: E402
from oracle import pyref as R  # noqa: E402
from test_msm_segments_host import SWITCHES, cuts, hseg  # noqa: F401  (hseg: the fixture that replays msm_segments.h)

CSRC = os.path.join(ROOT, "mathlib_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    return G.all_cases()


def _header(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+[\w:]+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "constant %s not found" % name
    return int(m.group(1))


def test_model_constants_match_the_headers():
    """A change of a threshold fails here and sends its author to the cases: each was built for the value the model holds."""
    sort, kern, acc, plan = _header("msm_sort.h"), _header("msm_kernels.h"), _header("msm_accumulate.h"), _header("msm_plan.h")
    seg = _header("msm_segments.h")
    assert _const(sort, "SORT_TILE") == G.SORT_TILE
    assert _const(sort, "SORT_TILE_MAX") == G.SORT_TILE_MAX
    assert _const(sort, "STAGE") == G.STAGE
    assert _const(sort, "BIGBIN_SLICE") == G.BIGBIN_SLICE
    assert _const(sort, "SCAN_TILE") == G.SCAN_TILE
    assert _const(acc, "BIG_SLICE") == G.BIG_SLICE
    assert _const(kern, "BIG_BUCKET_MIN") == G.BIG_BUCKET_MIN
    assert _const(kern, "QUAD_ACC_MAX_BUCKETS") == G.QUAD_ACC_MAX_BUCKETS
    m = re.search(r"kLdsMax\s*=\s*(\d+)\s*\*\s*(\d+)\s*-\s*(\d+)\s*;", plan)
    assert m and int(m.group(1)) * int(m.group(2)) - int(m.group(3)) == G.LDS_MAX
    m = re.search(r"big_bin\s*=.*std::max<size_t>\((\d+),\s*(\d+)\s*\*\s*\(\(size_t\)Wd\s*\*\s*n\s*/\s*NB\)\)", plan)
    assert m and (int(m.group(1)), int(m.group(2))) == (G.BIGBIN_FLOOR, G.BIGBIN_FACTOR)
    # the accepted tiles and the default by n, the bin limit, the fine-bucket bits, the threshold of the long buckets
    assert re.search(r"v == 1024 \|\| v == 2048 \|\| v == 4096 \|\| v == 8192", sort) and G.SORT_TILES == (1024, 2048, 4096, 8192)
    assert re.search(r"n >= \(\(size_t\)1 << 23\)\) return 8192;\s*if \(n >= \(\(size_t\)1 << 22\)\) return 4096;\s*"
                     r"if \(n >= \(\(size_t\)1 << 20\)\) return 2048;", sort)
    assert re.search(r"int low = p->c - 1 < %d \? p->c - 1 : %d;" % (G.SORT_LOW_MAX, G.SORT_LOW_MAX), plan)
    assert re.search(r"nb > %d" % G.SORT_NB_MAX, plan)
    assert re.search(r"while \(t > 1024 && staged_lds\(t\) > kLdsMax\) t /= 2;", plan)
    assert re.search(r"return \(3 \* \(size_t\)NB \+ \(size_t\)t \* Wd\) \* 4;", plan)
    assert re.search(r"while \(group < 64 && \(size_t\)group \* 2 \* NB <= \(size_t\)tile \* Wd\) group \*= 2;", plan)
    assert re.search(r">> \(p->c - 1\)\) \* %d, 1u << 30\)" % G.BIG_THRESHOLD_FACTOR, plan)
    assert re.search(r"#define MLHIP_MAX_SEGMENTS %d\b" % G.MAX_SEGMENTS, seg)


def _hm_digits(hostmath, cid, scalar, c):
    out = (ctypes.c_uint32 * 80)()
    W = hostmath.hm_digits(cid, int(scalar).to_bytes(32, "little"), 0, c, out, 80)
    return [(-1 if out[w] & 1 else 1) * (out[w] >> 1) for w in range(W)]


@pytest.mark.parametrize("curve", G.CURVES)
def test_digit_replica_against_the_kernel_body(hostmath, curve, cases):
    """digits() against msm_digits_body compiled for the host: per c, hand-picked edges, the scalars of every case of the
    curve (a sample of 2500 of them where there are more) and unreduced values."""
    cp = R.CURVES[curve]
    rng = np.random.default_rng(11 + cp.curve_id)
    for c in (9, 13, 16):
        W, widths, offs = G.win_layout(curve, c)
        pool = [0, 1, cp.r - 1, cp.r - 2, (1 << c) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, cp.r, cp.r + 5, (1 << 256) - 1]
        pool += [((1 << (offs[k] + widths[k])) - 1) % cp.r for k in (0, W // 2, W - 2)]
        mine = [s for case in cases if case.curve == curve and any(rc == c for _, rc, _, _ in case.runs) for s in case.scalars]
        mine = sorted(set(mine))
        if len(mine) > 2500:
            mine = [mine[i] for i in rng.choice(len(mine), size=2500, replace=False)]
        pool += mine + [int.from_bytes(rng.bytes(32), "little") % cp.r for _ in range(2000 - min(2000, len(mine)))]
        assert len(pool) >= 2000
        got = G.digits(curve, c, pool)
        for s, row in zip(pool, got):
            assert list(row) == _hm_digits(hostmath, cp.curve_id, s, c), (curve, c, hex(s))


@pytest.mark.parametrize("curve", G.CURVES)
def test_scalar_from_digits_gives_the_digits_back(hostmath, curve):
    cp = R.CURVES[curve]
    rng = np.random.default_rng(23 + cp.curve_id)
    for c in (9, 13, 16):
        rows = G.random_rows(curve, c, 300, rng)
        rows[::7, 1] = -rows[::7, 1]
        rows[::5, 2] = 0
        for w in range(rows.shape[1] - 1):  # the extremes of a window's range
            lo, hi = G.digit_range(G.win_layout(curve, c)[1][w])
            rows[w, w], rows[100 + w, w] = lo, hi
        scalars = G.scalars_from_rows(curve, c, rows)
        assert (G.digits(curve, c, scalars) == rows).all()
        for s, row in list(zip(scalars, rows))[:60]:
            assert G.scalar_from_digits(curve, c, row) == s
            assert _hm_digits(hostmath, cp.curve_id, s, c) == list(row)


def test_every_claimed_fact_holds_in_the_model(cases):
    """For every case and every way it is run: each fact the case claims, asserted from the model of exactly that run."""
    checked = 0
    for case in cases:
        assert case.runs, case.name
        assert all(0 < s < R.CURVES[case.curve].r for s in case.scalars), case.name
        for label, c, switches, facts in case.runs:
            m = case.model(c, switches)
            assert facts, (case.name, label)
            for fact in facts:
                G.check_fact(m, fact)
                checked += 1
    assert checked > 500


def test_the_cases_cover_the_edges_between_them(cases):
    """What the set as a whole must contain (the issue's list), read from the models."""
    runs = [(case, label, c, sw, case.model(c, sw)) for case in cases for label, c, sw, _ in case.runs]
    sorts = [(case, label, m["seg"][0]["sort"]) for case, label, c, sw, m in runs if not m["streams"]]
    two = [s for _, _, s in sorts if s["path"] == "two-level"]
    assert any(s["path"] == "legacy" for _, _, s in sorts)
    # tiles: staged at 2048, unstaged at 8192, a staged request the LDS bound shrinks back to 1024, two group sizes, ragged blocks
    assert any(s["staged"] and s["tile"] == 2048 for s in two)
    assert any(not s["staged"] and s["tile"] == 8192 for s in two)
    assert any(s["staged"] and s["tile_asked"] > 1024 and s["tile"] == 1024 for s in two)
    assert len({s["group"] for s in two if s["staged"]}) >= 3
    assert any(s["tile"] > 1024 and s["n"] % s["tile"] == 1 for s in two) and any(s["n"] % s["tile"] == s["tile"] - 1 for s in two)
    # k_fine_sort: STAGE and STAGE + 1; the multi-workgroup bins: big_bin and big_bin + 1, a multiple of the slice, a bin at
    # an index of 1024 or more, a bin of one fine bucket and one of 256, big_bin from the mean
    counts = {(int(cnt), s["paths"][b][0]) for s in two for b, cnt in enumerate(s["bin_counts"]) if cnt}
    assert (G.STAGE, "staged") in counts and (G.STAGE + 1, "direct") in counts
    assert any(p == ("multi", [G.BIGBIN_SLICE] * 3) for s in two for p in s["paths"].values())
    for origin in ("floor", "mean"):
        ss = [s for s in two if s["big_bin_from"] == origin]
        assert any(int(cnt) == s["big_bin"] and s["paths"][b][0] == "direct" for s in ss for b, cnt in enumerate(s["bin_counts"]) if cnt)
        assert any(int(cnt) == s["big_bin"] + 1 and s["paths"][b][0] == "multi" for s in ss for b, cnt in enumerate(s["bin_counts"]) if cnt)
    assert any(b >= 1024 and p[0] == "multi" for s in two for b, p in s["paths"].items())
    assert any(sum(p[0] == "multi" for p in s["paths"].values()) >= 3 for s in two)
    # long buckets: 256 / 257, the slice boundaries, more than 1024 of them, the gate of the one-pass launches
    accs = [m["seg"][0]["acc"] for case, label, c, sw, m in runs if not m["streams"]]
    lens = {tuple(v) for a in accs for v in a["long"].values()}
    for want in ([257], [4096], [4096, 1], [4096, 4096], [4096, 4096, 1]):
        assert tuple(want) in lens, want
    assert any(not a["long_step"] for a in accs) and any(len(a["long"]) > 1024 for a in accs)
    assert any(a["quad"] and a["long"] for a in accs) and any(not a["quad"] and a["long"] for a in accs)
    assert any(a["big_threshold"] > G.BIG_BUCKET_MIN and a["long"] for a in accs)


@pytest.mark.parametrize("group", [1, 2])
def test_segment_cuts_of_the_segmented_cases(hseg, group, monkeypatch):  # noqa: F811
    """The model's cuts against msm_segments.h itself: a host-buffer call under MLHIP_STREAM_SEGMENTS = 3 and a device-resident
    plan under MLHIP_TILE_LOG2 = 11 are both cut at 2000 and 4000, for G1 and G2 alike."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    assert G.SEG_N % G.SEG_K == 0
    case = G.long_segments("BLS12-381", group)
    m = case.model(G.SEG_C, {"segments": G.SEG_K})
    assert m["streams"] and m["bounds"] == [0, 2000, 4000, 6000]
    monkeypatch.setenv("MLHIP_STREAM_SEGMENTS", str(G.SEG_K))
    assert cuts(hseg, group, G.SEG_N, "both")[0] == m["bounds"]
    monkeypatch.delenv("MLHIP_STREAM_SEGMENTS")
    monkeypatch.setenv("MLHIP_TILE_LOG2", "11")
    for edwards in (False, True):
        assert cuts(hseg, group, G.SEG_N, "resident", edwards=edwards)[0] == m["bounds"]
    assert G.equal_cuts(7, 3) == [0, 3, 6, 7] and G.equal_cuts(6000, 24)[-2:] == [5750, 6000]


def case_table(cases):
    lines = []
    for case in cases:
        for label, c, switches, facts in case.runs:
            sw = ",".join("%s=%s" % kv for kv in sorted(switches.items())) or "-"
            lines.append("%s %s G%d n=%d c=%d %s [%s]" % (case.name, case.curve, case.group, case.n, c, sw, label))
            lines += ["    " + repr(f) for f in facts]
    return lines


def test_case_table_lists_every_run(cases):
    table = case_table(cases)
    assert sum(not line.startswith("    ") for line in table) == sum(len(case.runs) for case in cases)


if __name__ == "__main__":
    print("\n".join(case_table(G.all_cases())))
