"""How an MSM is cut into segments and tiles, without a GPU: mathlib_amd/csrc/msm_segments.h compiled with g++
(tests/hostmath_segments) and asked through ctypes, the way api_msm.hip / api_bases.hip / msm_plan.h ask it.  Invariants of
the cuts over a sweep of sizes, groups, plan kinds, protocols and MLHIP_* switches; a few cuts worked out by hand; and the
whole sweep against tests/golden/msm_segments.json, recorded from the functions as they were moved out of msm_plan.h and
api_msm.hip -- a later edit of the policy shows up as a diff of that file
(MLHIP_RECORD_SEGMENTS=1 pytest tests/test_msm_segments_host.py rewrites it)."""
import ctypes
import json
import os
import subprocess

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "msm_segments.json")
SIZES = [1, 2, 1023, 1024, 1025, 1 << 16, 3 * (1 << 16) + 5, (1 << 17) - 1, 1 << 20, 1 << 21, (1 << 22) + 7, 1 << 24, 1 << 27]
ENVS = ([{}] + [{"MLHIP_STREAM_SEGMENTS": str(v)} for v in (1, 2, 5, 24, 99)]
        + [{"MLHIP_STREAM_SCHEDULE": v} for v in ("1,1,2", "3,13", "7")] + [{"MLHIP_TILE_LOG2": str(v)} for v in (0, 10, 16, 40)])
SWITCHES = ("MLHIP_STREAM_SEGMENTS", "MLHIP_STREAM_SCHEDULE", "MLHIP_TILE_LOG2")
# what travels per call: nothing (device-resident inputs), the scalars (resident bases), scalars and points (host buffers)
PROTOCOLS = ("resident", "scalars", "both")
FOLD_TILES = (0, 1 << 16, 1 << 20)  # 0: a plain plan
EINVAL_TILES = "EINVAL: too many tiles"


@pytest.fixture(scope="module")
def hseg():
    d = os.path.join(ROOT, "tests", "hostmath_segments")
    so = os.path.join(d, "libsegments_host.so")
    src = os.path.join(d, "segments_host.cpp")
    hdr = os.path.join(ROOT, "mathlib_amd", "csrc", "msm_segments.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    sz, i = ctypes.c_size_t, ctypes.c_int
    lib.hseg_resident_tiles.argtypes = [i, i, i, sz, i, sz]
    lib.hseg_stream_segments.argtypes = [i, i, sz]
    lib.hseg_shared_segments.argtypes = [i, sz]
    lib.hseg_train.argtypes = [i, sz, i, i, i, sz, i, i, i, i, ctypes.POINTER(sz), ctypes.POINTER(i), ctypes.POINTER(sz)]
    return lib


def train(hseg, group, n, K, fold_tile=0, scalars_travel=False, points_travel=False, edwards=False, shared=False):
    """The bounds and the longest segment of a train of K segments (msm_plan.h: plan_stream_train), or the
    library's error."""
    bound = (ctypes.c_size_t * (hseg.hseg_max_segments() + 1))()
    k, seg = ctypes.c_int(0), ctypes.c_size_t(0)
    rc = hseg.hseg_train(group == 1, n, K, 1 if shared else 2, 1 if fold_tile else 0, fold_tile, scalars_travel, points_travel,
                         edwards, shared, bound, ctypes.byref(k), ctypes.byref(seg))
    assert rc in (0, 2), rc  # ("bad segment count": the callers below never ask for fewer than min_K segments)
    if rc == 2:
        return EINVAL_TILES, 0
    return list(bound[: k.value + 1]), seg.value


def cuts(hseg, group, n, protocol, fold_tile=0, edwards=False):
    """One MSM of n pairs, as the entry points route it: mlhip_msm_run / mlhip_bases_msm_device ("resident"), mlhip_bases_msm
    once the bases are converted ("scalars"), mlhip_msm_g1 / _g2 ("both").  A call that is not streamed is one pass, unless
    its points are resident and plan_launch cuts it into tiles."""
    fold = 1 if fold_tile else 0
    if protocol != "resident":
        K = hseg.hseg_stream_segments(1, group == 1, n)
        if K > 1:
            return train(hseg, group, n, K, fold_tile, True, protocol == "both", edwards)
        if protocol == "both":
            return [0, n], n  # (the points ride the auxiliary stream of the one pass)
    K = hseg.hseg_resident_tiles(1, group == 2, fold, fold_tile, edwards, n)
    return train(hseg, group, n, K, fold_tile, edwards=edwards) if K > 1 else ([0, n], n)


def sweep():
    for env in ENVS:
        for group in (1, 2):
            for fold_tile in FOLD_TILES:
                for protocol in PROTOCOLS:
                    if fold_tile and protocol == "both":
                        continue  # the points of a folded plan are its table: they never travel
                    for n in SIZES:
                        yield env, group, fold_tile, protocol, n


def key(env, group, fold_tile, protocol, n):
    e = ",".join("%s=%s" % kv for kv in env.items()) or "-"
    return "%s G%d fold_tile=%d %s n=%d" % (e, group, fold_tile, protocol, n)


@pytest.fixture(scope="module")
def swept(hseg):
    """key -> (bounds or the error, longest segment) for the whole sweep, computed once"""
    saved = {s: os.environ.pop(s, None) for s in SWITCHES}
    out = {}
    try:
        for env, group, fold_tile, protocol, n in sweep():
            os.environ.update(env)
            out[key(env, group, fold_tile, protocol, n)] = cuts(hseg, group, n, protocol, fold_tile)
            for s in env:
                del os.environ[s]
    finally:
        for s, v in saved.items():
            if v is not None:
                os.environ[s] = v
    return out


def test_invariants_of_every_cut(hseg, swept):
    kmax = hseg.hseg_max_segments()
    assert kmax == 24
    for env, group, fold_tile, protocol, n in sweep():
        k = key(env, group, fold_tile, protocol, n)
        bounds, seg = swept[k]
        if bounds == EINVAL_TILES:  # the documented refusal: a folded plan whose table has more tiles than segments allowed
            assert fold_tile and -(-n // fold_tile) > kmax, k
            continue
        assert not (fold_tile and -(-n // fold_tile) > kmax and len(bounds) > 2), k
        K = len(bounds) - 1
        assert 1 <= K <= kmax, k
        assert bounds[0] == 0 and bounds[K] == n, k
        assert all(a < b for a, b in zip(bounds, bounds[1:])), k
        assert seg == max(b - a for a, b in zip(bounds, bounds[1:])), k
        if fold_tile and K > 1:  # no segment has a multiple of fold_tile in its interior
            for a, b in zip(bounds, bounds[1:]):
                assert (b - 1) // fold_tile == a // fold_tile, (k, a, b)


def test_growing_schedule_of_resident_bases(hseg, monkeypatch):
    """Resident bases, G1, the scalars travel, the points do not, tile 2^21: 3 x 2^16 pairs, then fourfold up to a tile."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    assert cuts(hseg, 1, 1 << 20, "scalars")[0] == [0, 196608, 1048576]
    assert cuts(hseg, 1, 1 << 21, "scalars")[0] == [0, 196608, 983040, 2097152]
    assert cuts(hseg, 1, 1 << 22, "scalars")[0] == [0, 196608, 983040, 3080192, 4194304]


def test_equal_segments_cut_at_the_tiles_of_a_folded_plan(hseg, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    n = 3 * (1 << 16) + 5
    bounds, seg = train(hseg, 1, n, 2, fold_tile=1 << 16)  # K = 2 equal segments: [0, 98307, n), then the cut
    assert bounds == [0, 65536, 98307, 131072, 196608, 196613]
    assert len(bounds) - 1 == 5 and seg == 65536


def encode(bounds):
    """Segment lengths, run-length coded: [0, 4, 8, 12, 13] -> "4*3 1"."""
    if bounds == EINVAL_TILES:
        return bounds
    runs = []
    for a, b in zip(bounds, bounds[1:]):
        if runs and runs[-1][0] == b - a:
            runs[-1][1] += 1
        else:
            runs.append([b - a, 1])
    return " ".join("%d*%d" % (l, c) if c > 1 else str(l) for l, c in runs)


def test_recorded_cuts(swept):
    """The sweep against the recorded results: switch -> plan and protocol -> n -> segment lengths.  Without a switch ("-")
    every cut that is not one pass is stored; under a switch, every cut that differs from the one without it."""
    got = {}
    for env, group, fold_tile, protocol, n in sweep():
        k = key(env, group, fold_tile, protocol, n)
        e, cfg = k.split(" ", 1)[0], k.split(" ", 1)[1].rsplit(" ", 1)[0]
        cut, base = encode(swept[k][0]), encode(swept[key({}, group, fold_tile, protocol, n)][0])
        if cut != (base if env else str(n)):
            got.setdefault(e, {}).setdefault(cfg, {})[str(n)] = cut
    if os.environ.get("MLHIP_RECORD_SEGMENTS") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=0, separators=(",", ":"))
            f.write("\n")
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for e in want:
        assert sorted(got[e]) == sorted(want[e]), e
        for cfg in want[e]:
            assert got[e][cfg] == want[e][cfg], (e, cfg)
