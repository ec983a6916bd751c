"""The MSM entry sort (msm_sort.h, launch_sort) and the long-bucket step (k_big_prefix, the slice kernels, accumulate_big_body,
launch_accumulate) at their geometry edges, through the public API, against cref.msm -- every assertion is byte equality of
the affine result.  A wrong rank, a dropped sign or a wrong prefix in these paths stays inside allocated buffers and changes
only the sum, so nothing else can see it.

The inputs and the model that says which branch each of them reaches are in tests/msm_geometry_cases.py; that they do reach
it is asserted on the CPU by tests/test_msm_geometry_host.py.  Only switches that exist are used: MLHIP_SORT_TILE,
MLHIP_SCATTER_STAGED, MLHIP_LEGACY_SORT, MLHIP_STREAM_SEGMENTS, MLHIP_TILE_LOG2, MLHIP_REDUCE32 (the test build) and
MLHIP_NO_PLAN_CACHE (the sort's parameters are fixed when a plan is created: no pooled plan)."""
import ctypes

import pytest

from conftest import load_golden  # noqa: F401  (puts the repository root on sys.path: the cases import the oracle)

import msm_geometry_cases as G  # noqa: E402
from oracle import pyref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CURVE_GROUPS = [(curve, group) for curve in G.CURVES for group in (1, 2)]
ENV_OF = {"sort_tile": "MLHIP_SORT_TILE", "segments": "MLHIP_STREAM_SEGMENTS"}


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def _set_switches(monkeypatch, switches):
    monkeypatch.setenv("MLHIP_NO_PLAN_CACHE", "1")
    for s in ("MLHIP_SORT_TILE", "MLHIP_SCATTER_STAGED", "MLHIP_LEGACY_SORT", "MLHIP_STREAM_SEGMENTS", "MLHIP_TILE_LOG2",
              "MLHIP_STREAM_SCHEDULE"):
        monkeypatch.delenv(s, raising=False)
    monkeypatch.setenv("MLHIP_STREAM_SEGMENTS", str(switches.get("segments", 0)))
    if "sort_tile" in switches:
        monkeypatch.setenv("MLHIP_SORT_TILE", str(switches["sort_tile"]))
    if not switches.get("staged", True):
        monkeypatch.setenv("MLHIP_SCATTER_STAGED", "0")
    if switches.get("legacy"):
        monkeypatch.setenv("MLHIP_LEGACY_SORT", "1")
    if switches.get("reduce32"):
        monkeypatch.setenv("MLHIP_REDUCE32", "1")  # (routes the rest of the test through the test build)


def _host_msm(lib, mlhip, case, c):
    cid = R.CURVES[case.curve].curve_id
    pts = case.points()
    out = ctypes.create_string_buffer(len(pts) // case.n)
    fn = lib.mlhip_msm_g1 if case.group == 1 else lib.mlhip_msm_g2
    mlhip.check(fn(cid, pts, case.scalar_raw(), 0, case.n, c, out))
    return out.raw


def _run_case(lib, mlhip, monkeypatch, case, only=None):
    """every host-buffer run of the case (or those whose label is in `only`) against the case's cref.msm"""
    want = case.expected()
    ran = 0
    for label, c, switches, _ in case.runs:
        if switches.get("edwards") or (only is not None and label not in only):
            continue
        _set_switches(monkeypatch, switches)
        assert _host_msm(lib, mlhip, case, c) == want, (case.name, case.curve, case.group, label)
        ran += 1
    assert ran


# ---- the sort -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [p for p, _ in G.SORT_PATHS])
@pytest.mark.parametrize("curve", G.CURVES)
def test_sort_composite(lib, mlhip, curve, path, monkeypatch):
    """c = 16, n = 32769: bins of big_bin and big_bin + 1 entries, of STAGE and STAGE + 1, three multi-workgroup bins with
    ordinary bins between them -- one of a single fine bucket, one of 256, one at bin 1252 with negative digits -- on the
    staged scatter, on the one-store-per-entry scatter and on the global-atomic sort"""
    _run_case(lib, mlhip, monkeypatch, G.sort_composite(curve), only=[path])


def test_sort_big_bin_of_three_full_slices(lib, mlhip, monkeypatch):
    _run_case(lib, mlhip, monkeypatch, G.sort_three_slices())


def test_sort_big_bin_set_by_the_mean(lib, mlhip, monkeypatch):
    """c = 13, n = 65552: big_bin = 32776 is 8 x the mean bin; bins of 32777 (sliced) and 32776 (one workgroup)"""
    _run_case(lib, mlhip, monkeypatch, G.sort_big_bin_from_mean())


@pytest.mark.parametrize("ragged", ["one", "short"])
@pytest.mark.parametrize("tile", [2048, 8192])
def test_sort_tiles(lib, mlhip, tile, ragged, monkeypatch):
    """MLHIP_SORT_TILE = 2048 / 8192 at n = tile + 1 and 2 tile - 1, c = 16 and 13, staged and unstaged: ragged last blocks,
    the tile / 1024 > 1 loop of the staged scatter, the 32 rounds of the unstaged one, a 16-bit block count of 8192"""
    _run_case(lib, mlhip, monkeypatch, G.sort_tile_case(tile, ragged))


# ---- the long buckets, one pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 257])
@pytest.mark.parametrize("curve,group", CURVE_GROUPS)
def test_long_all_equal(lib, mlhip, curve, group, n, monkeypatch):
    """n = 256: every bucket at BIG_BUCKET_MIN, no long-bucket launch; n = 257: every bucket sliced (c = 9: G1 on quads)"""
    for c in G.LONG_C:
        _run_case(lib, mlhip, monkeypatch, G.long_all_equal(curve, group, n, c))


@pytest.mark.parametrize("curve,group", CURVE_GROUPS)
def test_long_buckets_side_by_side(lib, mlhip, curve, group, monkeypatch):
    """buckets of 256, 257, 4096, 4097 (G1: 8192, 8193) entries of distinct points in one window"""
    for c in G.LONG_C:
        _run_case(lib, mlhip, monkeypatch, G.long_side_by_side(curve, group, c))


@pytest.mark.parametrize("curve,group", [(curve, 1) for curve in G.CURVES] + [("BLS12-381", 2)])
def test_more_than_1024_long_buckets(lib, mlhip, curve, group, monkeypatch):
    """1040 long buckets, 1040 slices: the second round of k_big_prefix and the grid strides of the slices and the combine"""
    _run_case(lib, mlhip, monkeypatch, G.long_many(curve, group))


@pytest.mark.parametrize("curve,group", CURVE_GROUPS)
def test_long_bucket_of_one_repeated_point(lib, mlhip, curve, group, monkeypatch):
    for c in G.LONG_C:
        _run_case(lib, mlhip, monkeypatch, G.long_repeated_point(curve, group, c))


@pytest.mark.parametrize("curve,group", CURVE_GROUPS)
def test_long_bucket_summing_to_infinity(lib, mlhip, curve, group, monkeypatch):
    for c in G.LONG_C:
        _run_case(lib, mlhip, monkeypatch, G.long_infinity(curve, group, c))


# ---- the long buckets across segments -------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", CURVE_GROUPS)
def test_long_buckets_across_segments(lib, mlhip, curve, group, monkeypatch):
    """three segments; buckets long in one and short or absent in the next (msm_geometry_cases.SEG_BUCKETS).  The model says
    that G2 streams on all three curves, so all three run."""
    _run_case(lib, mlhip, monkeypatch, G.long_segments(curve, group), only=["segments"])


@pytest.mark.parametrize("curve", G.CURVES)
def test_long_buckets_across_segments_reduce32(lib, mlhip, curve, monkeypatch):
    """the boundary-form reduction (test build): the last segment leaves d_buckets, from accumulate_seg_body's conversion of
    the kept state or, for a bucket that is long in the last segment, from the combine's `buckets[g] = sum`"""
    _run_case(lib, mlhip, monkeypatch, G.long_segments(curve, 1), only=["reduce32"])


def test_long_buckets_across_tiles_edwards(lib, mlhip, monkeypatch):
    """a BLS12-377 plan with the SRS promise cut into three tiles: the same crossings on the Edwards state"""
    import torch

    case = G.long_segments("BLS12-377", 1)
    assert any(sw.get("edwards") for _, _, sw, _ in case.runs)
    _set_switches(monkeypatch, {})
    monkeypatch.setenv("MLHIP_TILE_LOG2", "11")
    dev = torch.device("cuda", 0)
    dp = torch.frombuffer(bytearray(case.points()), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(case.scalar_raw()), dtype=torch.uint8).to(dev)
    plan = mlhip.MsmPlan(R.CURVES[case.curve].curve_id, 1, case.n, G.SEG_C)
    try:
        plan.set_profiling(True)
        plan.assume_srs(True)
        got = plan.run(dp.data_ptr(), ds.data_ptr(), case.n, False, torch.cuda.current_stream().cuda_stream)
        t = plan.timings()
        assert t["edwards"] == 1.0 and t["tiles"] == float(G.SEG_K), t
        assert got == case.expected()
    finally:
        plan.close()
