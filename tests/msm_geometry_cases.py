"""The geometry of the MSM entry sort (msm_sort.h, launch_sort in msm_plan.h) and of the long-bucket step (k_big_prefix, the
slice kernels, accumulate_big_body, launch_accumulate), modelled in plain Python, and the inputs that reach its edges.

The library does not report which sort path ran or which bucket went to the long-bucket step.  So the tests split the
question: tests/test_msm_geometry_host.py asserts from this model, on the CPU, that an input reaches the branch it was
built for (and that the model's constants are still those of the headers); tests/test_msm_geometry_gpu.py runs the same
input through the public API and compares the affine result with cref.msm, byte for byte.

Three parts:
  the digit replica   win_layout / digits: msm_win_layout and msm_window_digit of msm_body.h, vectorised over the scalars
  the model           model(): the host-side choices of plan_alloc_sort, launch_sort, big_bucket_threshold and
                      launch_accumulate for (curve, group, c, scalars, switches), per segment for a segmented run
  the cases           scalar_from_digits and the builders; a case holds its scalars, the recipe of its points and the facts it
                      claims (check_fact asserts one fact from the model)

The model always recomputes the digits from the finished scalars: the digits a builder asked for are never trusted."""
import numpy as np

from oracle import pyref as R

CURVES = ["BN254", "BLS12-381", "BLS12-377"]

# ---- the constants the model holds (tests/test_msm_geometry_host.py compares them with the headers) ---------------------
SORT_TILE = 1024
SORT_TILE_MAX = 8192
SORT_TILES = (1024, 2048, 4096, 8192)  # what MLHIP_SORT_TILE accepts
STAGE = 10240  # k_fine_sort: entries of a bin whose sorted image is assembled in LDS
BIGBIN_SLICE = 16384
BIGBIN_FLOOR = 32768  # big_bin = max(this, BIGBIN_FACTOR x the mean bin)
BIGBIN_FACTOR = 8
SORT_NB_MAX = 4096  # more coarse bins than this: the global-atomic sort
SORT_LOW_MAX = 8
LDS_MAX = 160 * 1024 - 256  # kLdsMax of launch_sort
SCAN_TILE = 4096
BIG_SLICE = 4096
BIG_BUCKET_MIN = 256
BIG_THRESHOLD_FACTOR = 8
QUAD_ACC_MAX_BUCKETS = 32768
MAX_SEGMENTS = 24


def fr_bits(curve):
    return R.CURVES[curve].r.bit_length()


# ---- the digit replica ---------------------------------------------------------------------------------------------------
def win_layout(curve, c):
    """msm_body.h: msm_win_layout -- the fr_bits + 1 bits spread over W windows whose widths differ by <= 1 (the replica of
    tests/test_host_math.py: _win_layout).  Returns (W, widths, offsets)."""
    total = fr_bits(curve) + 1
    W = (total + c - 1) // c
    base, rem = divmod(total, W)
    widths = [base + 1 if w < rem else base for w in range(W)]
    offs = [sum(widths[:w]) for w in range(W)]
    assert max(widths) <= c and max(widths) - min(widths) <= 1 and offs[-1] + widths[-1] == total
    return W, widths, offs


def scalar_bytes(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def digits(curve, c, scalars):
    """msm_window_digit over all windows of every scalar: an int64 array [n, W] of signed digits (0 = no entry; otherwise the
    entry goes to bucket |d| - 1 of its window with the sign of d).  A value of r or more is reduced first, as fr_canonical
    does."""
    r = R.CURVES[curve].r
    W, widths, offs = win_layout(curve, c)
    n = len(scalars)
    raw = np.frombuffer(scalar_bytes([int(s) % r for s in scalars]), dtype=np.uint8).reshape(n, 32)
    bits = np.unpackbits(raw, axis=1, bitorder="little").astype(np.int64)
    out = np.zeros((n, W), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(W):
        hi = min(offs[w] + widths[w], 256)
        v = bits[:, offs[w]:hi] @ (np.int64(1) << np.arange(hi - offs[w], dtype=np.int64)) + carry
        neg = v > (1 << (widths[w] - 1))  # (v == 2^width is digit 0 with a carry)
        out[:, w] = np.where(neg, v - (1 << widths[w]), v)
        carry = neg.astype(np.int64)
    assert not carry.any(), "the extra bit of the layout absorbs the last carry"
    return out


def digit_range(width):
    """what msm_window_digit can return for a window of this width: [-(2^(width-1) - 1), 2^(width-1)]"""
    return -((1 << (width - 1)) - 1), 1 << (width - 1)


def scalar_from_digits(curve, c, row):
    """The scalar whose signed window digits are `row` (one per window).  Every digit is in the range the device produces, the
    top non-zero digit is positive and the value is below r: the decomposition is unique, so the device gives `row` back."""
    W, widths, offs = win_layout(curve, c)
    assert len(row) == W
    v = 0
    for w in range(W):
        d = int(row[w])
        lo, hi = digit_range(widths[w])
        assert lo <= d <= hi, (w, d)
        v += d << offs[w]
    top = [int(d) for d in row if int(d) != 0]
    assert top and top[-1] > 0 and 0 < v < R.CURVES[curve].r
    return v


def random_rows(curve, c, n, rng):
    """n rows of uniformly random digits; the top digit in [1, (r >> off) - 2], so that whatever the windows below are changed
    to, the value stays positive and below r"""
    W, widths, offs = win_layout(curve, c)
    rows = np.zeros((n, W), dtype=np.int64)
    for w in range(W - 1):
        lo, hi = digit_range(widths[w])
        rows[:, w] = rng.integers(lo, hi + 1, size=n)
    top = (R.CURVES[curve].r >> offs[W - 1]) - 2
    assert top >= 1
    rows[:, W - 1] = rng.integers(1, top + 1, size=n)
    return rows


def scalars_from_rows(curve, c, rows):
    """scalar_from_digits for every row of an int64 array [n, W]"""
    W, widths, offs = win_layout(curve, c)
    rows = np.asarray(rows, dtype=np.int64)
    assert rows.shape[1] == W
    vals = np.zeros(len(rows), dtype=object)
    top = np.zeros(len(rows), dtype=np.int64)
    for w in range(W):
        lo, hi = digit_range(widths[w])
        assert (rows[:, w] >= lo).all() and (rows[:, w] <= hi).all(), w
        vals = vals + rows[:, w].astype(object) * (1 << offs[w])
        top = np.where(rows[:, w] != 0, rows[:, w], top)
    assert (top > 0).all()
    out = [int(v) for v in vals]
    assert 0 < min(out) and max(out) < R.CURVES[curve].r
    return out


# ---- the model -----------------------------------------------------------------------------------------------------------
def _slices(count, size):
    return [size] * (count // size) + ([count % size] if count % size else [])


def default_sort_tile(n):
    """sort_tile_for without MLHIP_SORT_TILE"""
    return 8192 if n >= 1 << 23 else 4096 if n >= 1 << 22 else 2048 if n >= 1 << 20 else 1024


def sort_model(c, W, max_n, dig, sort_tile=None, staged_on=True, legacy=False):
    """plan_alloc_sort and launch_sort for one sort of len(dig) scalars in buffers made for max_n"""
    n = len(dig)
    M = 1 << (c - 1)
    nbuckets = W * M
    idx_bits = 1
    while (1 << idx_bits) < max_n:
        idx_bits += 1
    low = min(c - 1, SORT_LOW_MAX, 31 - idx_bits)
    nb = nbuckets >> low if low >= 1 else 0
    mag = np.abs(dig)
    g = np.where(mag > 0, np.arange(W, dtype=np.int64)[None, :] * M + mag - 1, -1)  # bucket of every entry, -1: none
    s = {"n": n, "idx_bits": idx_bits, "entry_bucket": g, "entry_neg": dig < 0,
         "bucket_counts": np.bincount(g[g >= 0], minlength=nbuckets)}
    if low < 1 or nb > SORT_NB_MAX or legacy:
        s["path"] = "legacy"  # k_digits / scan / k_scatter
        return s
    tile = sort_tile if sort_tile in SORT_TILES else default_sort_tile(n)
    s["tile_asked"] = tile

    def staged_lds(t):
        return (3 * nb + t * W) * 4

    staged = False
    if staged_on:
        t = tile
        while t > 1024 and staged_lds(t) > LDS_MAX:
            t //= 2
        if staged_lds(t) <= LDS_MAX:
            tile, staged = t, True
    group = None
    if staged:
        group = 1
        while group < 64 and group * 2 * nb <= tile * W:
            group *= 2
    big_bin = min(max(BIGBIN_FLOOR, BIGBIN_FACTOR * (W * n // nb)), 0x7FFFFFFF)
    bin_counts = s["bucket_counts"].reshape(nb, 1 << low).sum(axis=1)
    paths = {}
    for b in np.nonzero(bin_counts)[0]:
        cnt = int(bin_counts[b])
        if cnt > big_bin:
            paths[int(b)] = ("multi", _slices(cnt, BIGBIN_SLICE))  # k_bigbin_hist / k_bigbin_place
        elif cnt <= STAGE:
            paths[int(b)] = ("staged", [cnt])  # k_fine_sort, the image in LDS
        else:
            paths[int(b)] = ("direct", [cnt])  # k_fine_sort, one store per entry
    s.update(path="two-level", low=low, NB=nb, tile=tile, staged=staged, group=group, blocks=-(-n // tile), big_bin=big_bin,
             big_bin_from="mean" if big_bin > BIGBIN_FLOOR else "floor", bin_counts=bin_counts, paths=paths,
             bigbin_launch=W * n > big_bin)
    assert s["bigbin_launch"] or not any(p[0] == "multi" for p in paths.values())
    return s


def acc_model(group, c, W, seg_len, bucket_counts, one_pass, reduce28):
    """big_bucket_threshold and launch_accumulate for one segment of seg_len scalars"""
    thr = max(BIG_BUCKET_MIN, min((seg_len >> (c - 1)) * BIG_THRESHOLD_FACTOR, 1 << 30))
    long_ = {int(g): _slices(int(bucket_counts[g]), BIG_SLICE) for g in np.nonzero(bucket_counts > thr)[0]}
    step = (not one_pass) or seg_len > thr  # k_big_prefix, the slices and the combine are launched
    assert step or not long_
    return {"big_threshold": thr, "long": long_, "long_step": step,
            "quad": group == 1 and one_pass and reduce28 and W * (1 << (c - 1)) <= QUAD_ACC_MAX_BUCKETS}


def equal_cuts(n, K):
    """segment_cuts without a schedule: K equal segments"""
    seg = -(-n // K)
    return list(range(0, n, seg)) + [n]


def model(curve, group, c, scalars, segments=0, tiles=False, sort_tile=None, staged=True, legacy=False, reduce32=False):
    """The geometry of one MSM.  segments >= 2: a host-buffer call under MLHIP_STREAM_SEGMENTS = segments, or (tiles) a
    device-resident plan cut into that many tiles by MLHIP_TILE_LOG2, whose sorts run in helper records sized for one tile.
    Every plan of this build has the carry-free copy and the auxiliary stream unless MLHIP_ACC32 is set, so G1 and G2 of all
    three curves stream.  Returns the plan's geometry and one {sort, acc} record per segment."""
    n = len(scalars)
    W, widths, offs = win_layout(curve, c)
    K = min(segments, MAX_SEGMENTS) if segments >= 2 and n >= segments else 1
    bounds = equal_cuts(n, K)
    dig = digits(curve, c, scalars)
    max_n = max(b - a for a, b in zip(bounds, bounds[1:])) if tiles and len(bounds) > 2 else n
    m = {"n": n, "W": W, "M": 1 << (c - 1), "nbuckets": W << (c - 1), "bounds": bounds, "streams": len(bounds) > 2, "seg": []}
    for a, b in zip(bounds, bounds[1:]):
        s = sort_model(c, W, max_n, dig[a:b], sort_tile, staged, legacy)
        acc = acc_model(group, c, W, b - a, s["bucket_counts"], not m["streams"], not reduce32)
        m["seg"].append({"sort": s, "acc": acc})
    return m


# ---- facts -----------------------------------------------------------------------------------------------------------------
def _bin_entries(s, b):
    """(scalar index, negative) of the entries of coarse bin b"""
    sel = (s["entry_bucket"] >> s["low"]) == b
    sel &= s["entry_bucket"] >= 0
    return np.nonzero(sel)[0], s["entry_neg"][sel]


def check_fact(m, fact):
    """Assert one claimed fact from the model.  A fact is a tuple (kind, arguments...); `seg` arguments index m["seg"]."""
    kind = fact[0]
    if kind == "sort":  # (kind, seg, {key: value}): host-side choices of the sort
        s = m["seg"][fact[1]]["sort"]
        for k, v in fact[2].items():
            assert s[k] == v, (fact, k, s[k])
    elif kind == "bin":  # (kind, seg, bin, count, path, slices)
        s = m["seg"][fact[1]]["sort"]
        assert int(s["bin_counts"][fact[2]]) == fact[3], (fact, int(s["bin_counts"][fact[2]]))
        assert s["paths"][fact[2]] == (fact[4], fact[5]), (fact, s["paths"][fact[2]])
    elif kind == "bin_fine":  # (kind, seg, bin, non-empty fine buckets, negative entries at least)
        s = m["seg"][fact[1]]["sort"]
        fine = s["bucket_counts"][fact[2] << s["low"]:(fact[2] + 1) << s["low"]]
        assert int((fine > 0).sum()) == fact[3], (fact, int((fine > 0).sum()))
        idx, neg = _bin_entries(s, fact[2])
        assert int(neg.sum()) >= fact[4] and (fact[4] == 0 or int((~neg).sum()) > 0), (fact, int(neg.sum()))
    elif kind == "bin_block_max":  # (kind, seg, bin, count): the most entries one block of `tile` scalars puts into the bin
        s = m["seg"][fact[1]]["sort"]
        idx, _ = _bin_entries(s, fact[2])
        assert int(np.bincount(idx // s["tile"]).max()) == fact[3], fact
    elif kind == "big_bins":  # (kind, seg, [bins]): exactly these go to the multi-workgroup path, ordinary bins between them
        s = m["seg"][fact[1]]["sort"]
        big = sorted(b for b, p in s["paths"].items() if p[0] == "multi")
        assert big == fact[2] and s["bigbin_launch"] == bool(big), (fact, big)
        for lo, hi in zip(big, big[1:]):
            assert any(lo < b < hi for b in s["paths"]), (fact, lo, hi)
    elif kind == "ragged":  # (kind, seg, blocks, scalars of the last block)
        s = m["seg"][fact[1]]["sort"]
        assert s["blocks"] == fact[2] and s["n"] - (s["blocks"] - 1) * s["tile"] == fact[3] and fact[3] < s["tile"], fact
    elif kind == "acc":  # (kind, seg, {key: value})
        a = m["seg"][fact[1]]["acc"]
        for k, v in fact[2].items():
            assert a[k] == v, (fact, k, a[k])
    elif kind == "bucket":  # (kind, seg, bucket, count, None | slices of the long bucket)
        sg = m["seg"][fact[1]]
        assert int(sg["sort"]["bucket_counts"][fact[2]]) == fact[3], (fact, int(sg["sort"]["bucket_counts"][fact[2]]))
        assert sg["acc"]["long"].get(fact[2]) == fact[4], (fact, sg["acc"]["long"].get(fact[2]))
        assert fact[4] is None or sg["acc"]["long_step"]
    elif kind == "long_totals":  # (kind, seg, long buckets at least, slices at least)
        a = m["seg"][fact[1]]["acc"]
        assert len(a["long"]) >= fact[2] and sum(len(v) for v in a["long"].values()) >= fact[3], (fact, len(a["long"]))
    elif kind == "plan":  # (kind, {key: value})
        for k, v in fact[1].items():
            assert m[k] == v, (fact, k, m[k])
    else:
        raise AssertionError("unknown fact %r" % (fact,))


# ---- cases -----------------------------------------------------------------------------------------------------------------
_BASE = {}


def base_points(curve, group, n):
    """the first n of the distinct points every case of (curve, group) draws from: cref.gen_points, P_i = [k0] G + i [k1] G,
    generated once at the size of the largest case; a uint8 array [n, point bytes]"""
    from oracle import cref

    have = _BASE.get((curve, group))
    if have is None or len(have) < n:
        size = max(n, MEAN_N if (curve, group) == ("BLS12-381", 1) else COMPOSITE_N if group == 1 else MANY_VALUES * MANY_REPEATS
                   if curve == "BLS12-381" else 9472)
        raw = cref.gen_points(R.CURVES[curve].curve_id, group, 0x5EED00 + 16 * CURVES.index(curve) + group, 0xA11CE, size)
        have = _BASE[(curve, group)] = np.frombuffer(raw, dtype=np.uint8).reshape(size, len(raw) // size)
    return have[:n]


class Case:
    """One input.  `point_of[i]` names the base point of pair i (an index into cref.gen_points(.., n_base)), `negated[i]` asks
    for its negative; `runs` lists the ways the GPU test runs it: (label, c, switches, facts).  The switches are those of
    model(): segments, tiles, sort_tile, staged, legacy, reduce32, and "edwards" for the plan with the SRS promise."""

    def __init__(self, name, curve, group, scalars, point_of=None, negated=None, seed=1):
        self.name, self.curve, self.group, self.scalars, self.n = name, curve, group, scalars, len(scalars)
        self.point_of = np.arange(self.n) if point_of is None else np.asarray(point_of)
        self.negated = np.zeros(self.n, dtype=bool) if negated is None else np.asarray(negated)
        self.seed = seed
        self.runs = []

    def run(self, label, c, facts, **switches):
        self.runs.append((label, c, switches, facts))

    def model(self, c, switches):
        key = (c, tuple(sorted(switches.items())))
        cache = self.__dict__.setdefault("_models", {})
        if key not in cache:
            kw = {k: v for k, v in switches.items() if k != "edwards"}
            cache[key] = model(self.curve, self.group, c, self.scalars, **kw)
        return cache[key]

    def points(self):
        """the points in the C ABI layout, built once"""
        if "_points" not in self.__dict__:
            from oracle import cref

            cp = R.CURVES[self.curve]
            rows = base_points(self.curve, self.group, int(self.point_of.max()) + 1)[self.point_of].copy()
            for i in np.nonzero(self.negated)[0]:
                p = bytes(rows[i])
                rows[i] = np.frombuffer(cref.point_mul(cp.curve_id, self.group, p, cp.r - 1), dtype=np.uint8)
            self._points = rows.tobytes()
        return self._points

    def scalar_raw(self):
        return scalar_bytes(self.scalars)

    def expected(self):
        """cref.msm of the whole input, computed once"""
        if "_expected" not in self.__dict__:
            from oracle import cref

            sc = np.frombuffer(self.scalar_raw(), dtype=np.uint64).reshape(self.n, 4)
            self._expected = cref.msm(R.CURVES[self.curve].curve_id, self.group, self.points(), sc, self.n, False, 0, 8)
        return self._expected


def _seed(curve, group, tag):
    return 100 * tag + 10 * CURVES.index(curve) + group


_CACHE = {}


def _cached(fn):
    def wrapped(*args):
        key = (fn.__name__,) + args
        if key not in _CACHE:
            _CACHE[key] = fn(*args)
        return _CACHE[key]

    wrapped.__name__ = fn.__name__
    return wrapped


# -- the sort -----------------------------------------------------------------------------------------------------------------
COMPOSITE_N = 32769
COMPOSITE_C = 16
SORT_PATHS = [("default", {}), ("unstaged", {"staged": False}), ("legacy", {"legacy": True})]


@_cached
def sort_composite(curve):
    """c = 16, n = 32769 = big_bin + 1 (big_bin at its floor): one scalar list whose windows are shaped one by one.
      w0  every entry in ONE bucket: a bin of big_bin + 1 entries holding one fine bucket (slices 16384, 16384, 1)
      w1  32768 entries in one bin, the last one elsewhere: exactly big_bin, the last bin on the single-workgroup path
      w2  every entry in one bin, spread over all 256 fine buckets, both signs
      w3  bins of 10240 (= STAGE) and 10241 entries (the second with both signs), the rest random
      w9  every entry in bin 100 of its window (bin 1252 of the sort: the second round of k_bigbin_prefix), two thirds of them
          negative, over 37 fine buckets
      all other windows uniformly random: ordinary bins between the big ones"""
    c, n = COMPOSITE_C, COMPOSITE_N
    W, widths, offs = win_layout(curve, c)
    assert W == 16 and all(wd == 16 for wd in widths[:10])
    rng = np.random.default_rng(1600 + CURVES.index(curve))
    rows = random_rows(curve, c, n, rng)
    i = np.arange(n)
    rows[:, 0] = 7
    rows[:, 1] = 3 * 256 + 50 * (i % 5) + 1
    rows[n - 1, 1] = 9 * 256 + 1
    rows[:, 2] = (17 * 256 + (i * 101) % 256 + 1) * np.where((i // 256) % 2 == 1, -1, 1)
    rows[:10240, 3] = 5 * 256 + (i[:10240] * 7) % 256 + 1
    rows[10240:20481, 3] = (6 * 256 + (i[10240:20481] * 11) % 256 + 1) * np.where(i[10240:20481] % 2 == 0, -1, 1)
    far = np.abs(rows[20481:, 3]) - 1  # keep the random rest of w3 out of the two pinned bins
    rows[20481:, 3] = np.where((far >> 8 == 5) | (far >> 8 == 6), 40 * 256 + 1, rows[20481:, 3])
    rows[:, 9] = (100 * 256 + (i * 5) % 37 + 1) * np.where(i % 3 != 0, -1, 1)
    case = Case("sort_composite", curve, 1, scalars_from_rows(curve, c, rows), seed=_seed(curve, 1, 1))
    bin_of = lambda w, coarse: (w << 7) + coarse  # noqa: E731  (c = 16: 128 coarse bins a window)
    facts = [
        ("sort", 0, {"path": "two-level", "low": 8, "NB": 2048, "big_bin": 32768, "big_bin_from": "floor", "tile": 1024,
                     "bigbin_launch": True}),
        ("bin", 0, bin_of(0, 0), n, "multi", [16384, 16384, 1]),
        ("bin_fine", 0, bin_of(0, 0), 1, 0),
        ("bin", 0, bin_of(1, 3), 32768, "direct", [32768]),
        ("bin_fine", 0, bin_of(1, 3), 5, 0),
        ("bin", 0, bin_of(1, 9), 1, "staged", [1]),
        ("bin", 0, bin_of(2, 17), n, "multi", [16384, 16384, 1]),
        ("bin_fine", 0, bin_of(2, 17), 256, 16000),
        ("bin", 0, bin_of(3, 5), 10240, "staged", [10240]),
        ("bin", 0, bin_of(3, 6), 10241, "direct", [10241]),
        ("bin_fine", 0, bin_of(3, 6), 256, 5000),
        ("bin", 0, bin_of(9, 100), n, "multi", [16384, 16384, 1]),
        ("bin_fine", 0, bin_of(9, 100), 37, 20000),
        ("big_bins", 0, [bin_of(0, 0), bin_of(2, 17), bin_of(9, 100)]),
    ]
    assert bin_of(9, 100) >= 1024
    case.run("default", c, facts + [("sort", 0, {"staged": True, "group": 8})])
    case.run("unstaged", c, facts + [("sort", 0, {"staged": False})], staged=False)
    case.run("legacy", c, [("sort", 0, {"path": "legacy"})], legacy=True)
    return case


@_cached
def sort_three_slices():
    """n = 49152 = 3 BIGBIN_SLICE with one window in a single bin: a big bin that is an exact multiple of the slice"""
    curve, c, n = "BLS12-381", 16, 49152
    rng = np.random.default_rng(4915)
    rows = random_rows(curve, c, n, rng)
    i = np.arange(n)
    rows[:, 5] = (64 * 256 + (i * 3) % 19 + 1) * np.where(i % 2 == 1, -1, 1)
    case = Case("sort_three_slices", curve, 1, scalars_from_rows(curve, c, rows), seed=2)
    b = (5 << 7) + 64
    case.run("default", c, [("sort", 0, {"big_bin": 32768, "big_bin_from": "floor"}),
                            ("bin", 0, b, n, "multi", [16384, 16384, 16384]), ("bin_fine", 0, b, 19, 20000), ("big_bins", 0, [b])])
    return case


MEAN_N = 65552
MEAN_C = 13


@_cached
def sort_big_bin_from_mean():
    """c = 13, n = 65552: 320 coarse bins of 4097 entries on average, so big_bin = 8 x 4097 = 32776 comes from the mean, not
    from the floor.  Window 1 puts 32777 entries into one bin (the first on the multi-workgroup path: slices 16384, 16384, 9),
    window 5 puts exactly 32776 into one (the last on the single-workgroup path)."""
    curve, c, n = "BLS12-381", MEAN_C, MEAN_N
    rng = np.random.default_rng(1313)
    rows = random_rows(curve, c, n, rng)
    i = np.arange(n)

    def pin(w, coarse, count, sign):
        far = np.abs(rows[:, w]) - 1
        rows[:, w] = np.where(far >> 8 == coarse, (coarse + 1) * 256 + 1, rows[:, w])  # nothing random in the pinned bin
        rows[:count, w] = (coarse * 256 + (i[:count] * 13) % 256 + 1) * sign[:count]

    pin(1, 3, 32777, np.where(i % 2 == 1, -1, 1))
    pin(5, 7, 32776, np.ones(n, dtype=np.int64))
    case = Case("sort_big_bin_from_mean", curve, 1, scalars_from_rows(curve, c, rows), seed=3)
    b1, b5 = (1 << 4) + 3, (5 << 4) + 7  # (c = 13: 16 coarse bins a window)
    case.run("default", c, [("sort", 0, {"NB": 320, "low": 8, "big_bin": 32776, "big_bin_from": "mean", "bigbin_launch": True}),
                            ("bin", 0, b1, 32777, "multi", [16384, 16384, 9]), ("bin_fine", 0, b1, 256, 16000),
                            ("bin", 0, b5, 32776, "direct", [32776]), ("big_bins", 0, [b1])])
    return case


TILE_RUNS = [(tile, c, staged) for tile in (2048, 8192) for c in (16, 13) for staged in (True, False)]


@_cached
def sort_tile_case(tile, ragged):
    """n = tile + 1 (ragged = "one": a last block of one scalar) or 2 tile - 1 (ragged = "short": a last block one scalar
    short) under MLHIP_SORT_TILE = tile: random scalars whose lowest window -- the low 13 bits hold the digit and bits 13..15
    are zero, so the same scalars serve c = 16 and c = 13 -- lies in bin 0: a full block counts `tile` entries for that bin in
    its 16-bit histogram.  What the launch makes of the request depends on c and on MLHIP_SCATTER_STAGED:
      c = 16  staged: 8192 shrinks to 2048 (155648 B of LDS; 4096 would need 286720), 16 lanes a bin; unstaged: 8192 stays
      c = 13  staged: 2048 and 8192 both shrink back to 1024 (2048 needs 167680 B > 163584), 64 lanes a bin"""
    curve = "BLS12-381"
    n = tile + 1 if ragged == "one" else 2 * tile - 1
    rng = np.random.default_rng(tile + n)
    r = R.CURVES[curve].r
    scalars = [((int.from_bytes(rng.bytes(32), "little") % (r >> 1)) >> 16 << 16) | (1 + i % 200) for i in range(n)]
    case = Case("sort_tile_%d_%s" % (tile, ragged), curve, 1, scalars, seed=4)
    for t, c, staged in TILE_RUNS:
        if t != tile:
            continue
        if staged:
            eff, group = (2048, 16) if c == 16 else (1024, 64)
        else:
            eff, group = tile, None
        blocks = -(-n // eff)
        facts = [("sort", 0, {"tile_asked": tile, "tile": eff, "staged": staged, "group": group, "blocks": blocks}),
                 ("ragged", 0, blocks, n - (blocks - 1) * eff), ("bin", 0, 0, n, "staged" if n <= STAGE else "direct", [n]),
                 ("bin_block_max", 0, 0, eff)]
        case.run("tile%d_c%d_%s" % (tile, c, "staged" if staged else "unstaged"), c, facts, sort_tile=tile, staged=staged)
    return case


# -- the long buckets, one pass ---------------------------------------------------------------------------------------------
LONG_C = (16, 9)


def _one_pass_facts(group, c, n):
    return [("plan", {"streams": False}), ("acc", 0, {"quad": group == 1 and c == 9})]


@_cached
def long_all_equal(curve, group, n, c):
    """all scalars equal, n = 256 (every bucket holds BIG_BUCKET_MIN entries: one lane each, and the one_pass gate skips the
    long-bucket launches) or 257 (every bucket is sliced: one slice of 257 entries, lane 0 adds two)"""
    W = win_layout(curve, c)[0]
    row = random_rows(curve, c, 1, np.random.default_rng(50 + c))[0]
    row[row == 0] = 3
    sc = scalar_from_digits(curve, c, row)
    facts = _one_pass_facts(group, c, n) + [("acc", 0, {"big_threshold": 256, "long_step": n > 256}),
                                            ("long_totals", 0, W if n > 256 else 0, W if n > 256 else 0)]
    for w in (0, W - 1):
        g = w * (1 << (c - 1)) + abs(int(row[w])) - 1
        facts.append(("bucket", 0, g, n, [n] if n > 256 else None))
    case = Case("long_all_equal_%d_c%d" % (n, c), curve, group, [sc] * n, seed=_seed(curve, group, 5))
    case.run("c%d" % c, c, facts)
    return case


def _pinned_window(curve, c, n, w, lengths, first_mag, rng, point_of=None):
    """rows of random digits whose window w holds buckets of the given lengths side by side from magnitude first_mag on (signs
    alternate inside a bucket), the other entries of the window kept away from them; the pairs are shuffled"""
    rows = random_rows(curve, c, n, rng)
    lo, hi = digit_range(win_layout(curve, c)[1][w])
    spare = np.arange(first_mag + len(lengths) + 8, hi)
    at = 0
    for k, ln in enumerate(lengths):
        rows[at:at + ln, w] = (first_mag + k) * np.where(np.arange(ln) % 3 == 1, -1, 1)
        at += ln
    assert at <= n
    rows[at:, w] = rng.choice(spare, size=n - at) * rng.choice([-1, 1], size=n - at)
    return rows, rng.permutation(n)


@_cached
def long_side_by_side(curve, group, c):
    """one window with buckets of 256, 257, 4096, 4097 (G1: and 8192, 8193) entries side by side, distinct points: the last
    bucket on one lane and the first sliced one, one and two full slices and a last slice of one entry (255 lanes of its tree
    at the identity).  At c = 9 the threshold is 8 x the mean, above 256: buckets of exactly that length and one more join."""
    lengths = [256, 257, 4096, 4097] + ([8192, 8193] if group == 1 else [])
    if c == 16:
        n = sum(lengths) + 100
        thr = 256
    else:
        n = {1: 26880, 2: 9472}[group]
        thr = (n >> 8) * 8
        lengths += [thr, thr + 1]
    rng = np.random.default_rng(7000 + 100 * c + _seed(curve, group, 0))
    w, first = 1, 10
    rows, order = _pinned_window(curve, c, n, w, lengths, first, rng)
    case = Case("long_side_by_side_c%d" % c, curve, group, scalars_from_rows(curve, c, rows[order]), seed=_seed(curve, group, 6))
    facts = _one_pass_facts(group, c, n) + [("acc", 0, {"big_threshold": thr, "long_step": True})]
    for k, ln in enumerate(lengths):
        facts.append(("bucket", 0, w * (1 << (c - 1)) + first + k - 1, ln, _slices(ln, BIG_SLICE) if ln > thr else None))
    case.run("c%d" % c, c, facts)
    return case


MANY_VALUES, MANY_REPEATS = 65, 257


@_cached
def long_many(curve, group):
    """65 scalar values 257 times each (n = 16705, c = 16), on distinct points: 65 x 16 = 1040 long buckets of one slice each --
    the second round of k_big_prefix, the grid stride of the 1024-block slice kernels and of the 256-block combine"""
    c = 16
    rng = np.random.default_rng(6500 + _seed(curve, group, 0))
    W = win_layout(curve, c)[0]
    while True:
        vals = random_rows(curve, c, MANY_VALUES, rng)
        if all(len(set(np.abs(vals[:, w]))) == MANY_VALUES and (vals[:, w] != 0).all() for w in range(W)):
            break
    n = MANY_VALUES * MANY_REPEATS
    rows = vals[np.arange(n) % MANY_VALUES]
    case = Case("long_many", curve, group, scalars_from_rows(curve, c, rows), seed=_seed(curve, group, 7))
    case.run("c16", c, _one_pass_facts(group, c, n) + [("acc", 0, {"big_threshold": 256, "long_step": True}),
                                                        ("long_totals", 0, 1025, 1025),
                                                        ("bucket", 0, abs(int(vals[0, 0])) - 1, 257, [257])])
    assert W * MANY_VALUES > 1024
    return case


@_cached
def long_repeated_point(curve, group, c):
    """a 4096-entry and a 4097-entry bucket of ONE point each (all entries positive): every lane of a slice holds the same
    partial sum, so every level of the LDS tree is a doubling; the 4097th entry is a slice of one"""
    lengths = [4096, 4097]
    n = sum(lengths) + 107
    rng = np.random.default_rng(8000 + 100 * c + _seed(curve, group, 0))
    w, first = 1, 20
    rows, order = _pinned_window(curve, c, n, w, lengths, first, rng)
    rows[:sum(lengths), w] = np.abs(rows[:sum(lengths), w])
    point_of = np.arange(n)
    point_of[:4096] = 0
    point_of[4096:8193] = 4096
    thr = max(256, (n >> (c - 1)) * 8)
    case = Case("long_repeated_point_c%d" % c, curve, group, scalars_from_rows(curve, c, rows[order]), point_of=point_of[order],
                seed=_seed(curve, group, 8))
    g0 = w * (1 << (c - 1)) + first - 1
    case.run("c%d" % c, c, _one_pass_facts(group, c, n) + [("acc", 0, {"big_threshold": thr}), ("bucket", 0, g0, 4096, [4096]),
                                                           ("bucket", 0, g0 + 1, 4097, [4096, 1])])
    return case


@_cached
def long_infinity(curve, group, c):
    """long buckets that sum to infinity: 300 entries of one point P, half under digit +d and half under -d of one window
    (the higher digits equal, so P is also a 300-entry bucket of one repeated point in every other window), and 160 distinct
    points each once under +e and once under -e.  Beside them P under a scalar s and under r - s, 100 times each: that pair
    cancels in the total only (r - s has other digits than s), not inside a bucket.  The rest is random pairs."""
    r = R.CURVES[curve].r
    n = 1300
    rng = np.random.default_rng(9000 + 100 * c + _seed(curve, group, 0))
    rows = random_rows(curve, c, n, rng)
    w, d, e = 1, 30, 31
    lo, hi = digit_range(win_layout(curve, c)[1][w])
    rows[:, w] = rng.integers(40, hi, size=n) * rng.choice([-1, 1], size=n)
    rows[:300] = rows[0]
    rows[:300, w] = d * np.where(np.arange(300) % 2 == 1, -1, 1)
    rows[300:620, w] = e * np.where(np.arange(320) % 2 == 1, -1, 1)
    point_of = np.arange(n)
    point_of[:300] = 0
    point_of[300:620] = 300 + np.arange(320) // 2
    scalars = scalars_from_rows(curve, c, rows)
    s = scalars[700]
    for k in range(100):
        scalars[620 + 2 * k], scalars[621 + 2 * k] = s, r - s
    point_of[620:820] = 0
    order = rng.permutation(n)
    case = Case("long_infinity_c%d" % c, curve, group, [scalars[i] for i in order], point_of=point_of[order],
                seed=_seed(curve, group, 9))
    base = w * (1 << (c - 1))
    case.run("c%d" % c, c, _one_pass_facts(group, c, n) + [("acc", 0, {"big_threshold": 256, "long_step": True}),
                                                           ("bucket", 0, base + d - 1, 300, [300]),
                                                           ("bucket", 0, base + e - 1, 320, [320])])
    return case


# -- the long buckets across segments -------------------------------------------------------------------------------------
SEG_N, SEG_K, SEG_C, SEG_W = 6000, 3, 16, 2
# bucket (magnitude in window SEG_W) -> entries per segment; 256 is the threshold of a 2000-scalar segment at c = 16
SEG_BUCKETS = {
    501: (300, 0, 5),    # long, absent, short: accumulate_big_body leaves the state accumulate_seg_body loads two segments on
    502: (5, 300, 0),    # short, long, absent: store_state -> state_to_boundary; the last segment finds nothing to add
    503: (0, 300, 280),  # absent, long, long: the first long segment meets the empty state
    504: (300, 3, 0),    # long but summing to infinity (150 points under +d and under -d), short, absent
    505: (0, 0, 300),    # long in the last segment only: under MLHIP_REDUCE32 the combine writes buckets[g] itself
    506: (4, 6, 290),    # short, short, long
    507: (300, 0, 0),    # long, then absent to the end: the kept state is all the last segment has
    508: (3, 0, 0),      # short, then absent to the end
}


@_cached
def long_segments(curve, group):
    """n = 6000 in three segments of 2000 (MLHIP_STREAM_SEGMENTS = 3 for the host-buffer calls; MLHIP_TILE_LOG2 = 11 cuts a
    device-resident plan at the same places), c = 16.  The buckets of SEG_BUCKETS live in window 2 and are long in one segment
    and short or absent in the next, so their sums cross between accumulate_big_body (state_to_boundary / boundary_to_state)
    and accumulate_seg_body (load_state / store_state) in both directions; the other windows are random."""
    c, n = SEG_C, SEG_N
    bounds = equal_cuts(n, SEG_K)
    rng = np.random.default_rng(3000 + _seed(curve, group, 0))
    rows = random_rows(curve, c, n, rng)
    lo, hi = digit_range(win_layout(curve, c)[1][SEG_W])
    rows[:, SEG_W] = rng.integers(1000, hi, size=n) * rng.choice([-1, 1], size=n)
    point_of = np.arange(n)
    negated = np.zeros(n, dtype=bool)
    for s, (a, b) in enumerate(zip(bounds, bounds[1:])):
        at = a
        for mag, counts in SEG_BUCKETS.items():
            k = counts[s]
            sign = np.where(np.arange(k) % 4 == 1, -1, 1)
            if mag == 504 and s == 0:  # pairs (Q, +d), (Q, -d): the bucket's sum is infinity
                sign = np.where(np.arange(k) % 2 == 1, -1, 1)
                point_of[at:at + k] = at + np.arange(k) // 2
            rows[at:at + k, SEG_W] = mag * sign
            at += k
        assert at <= b
        order = a + rng.permutation(b - a)
        rows[a:b], point_of[a:b] = rows[order], point_of[order]
    case = Case("long_segments", curve, group, scalars_from_rows(curve, c, rows), point_of=point_of, negated=negated,
                seed=_seed(curve, group, 10))
    facts = [("plan", {"streams": True, "bounds": bounds})]
    for s in range(SEG_K):
        facts.append(("acc", s, {"big_threshold": 256, "long_step": True, "quad": False}))
        for mag, counts in SEG_BUCKETS.items():
            g = SEG_W * (1 << (c - 1)) + mag - 1
            facts.append(("bucket", s, g, counts[s], [counts[s]] if counts[s] > 256 else None))
    case.run("segments", c, facts, segments=SEG_K)
    if group == 1:
        case.run("reduce32", c, facts, segments=SEG_K, reduce32=True)
        if curve == "BLS12-377":
            case.run("edwards_tiles", c, facts, segments=SEG_K, tiles=True, edwards=True)
    return case


def all_cases():
    """every case of the two test files, built once per process"""
    out = [sort_composite(curve) for curve in CURVES] + [sort_three_slices(), sort_big_bin_from_mean()]
    out += [sort_tile_case(tile, ragged) for tile in (2048, 8192) for ragged in ("one", "short")]
    for curve in CURVES:
        for group in (1, 2):
            for c in LONG_C:
                out += [long_all_equal(curve, group, 256, c), long_all_equal(curve, group, 257, c)]
                out += [long_side_by_side(curve, group, c), long_repeated_point(curve, group, c), long_infinity(curve, group, c)]
            if group == 1 or curve == "BLS12-381":
                out.append(long_many(curve, group))
            out.append(long_segments(curve, group))
    return out
