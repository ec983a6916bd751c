// msm_segments.h -- how an MSM is cut into segments / tiles: plain integer arithmetic on (group, n, the plan's fold_tile, a
// few flags, the MLHIP_* switches), without a HIP type, so that tests/hostmath_segments replays it on the CPU
// (tests/test_msm_segments_host.py; the recorded cuts are tests/golden/msm_segments.json).  The train that runs the
// segments is in msm_plan.h (plan_stream_train); api_msm.hip and api_bases.hip ask stream_segments.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

#define MLHIP_MAX_SEGMENTS 24

namespace mlhip {

// the cuts of one streamed / tiled MSM (the part of msm_plan.h's StreamCtx that is policy)
struct SegmentCuts {
  size_t n = 0, seg = 0;  // seg: the longest segment (what a sort-ahead record must hold)
  int K = 0;
  size_t bound[MLHIP_MAX_SEGMENTS + 1] = {};  // segment s = pairs [bound[s], bound[s + 1])
  bool scheduled = false;                     // bound[] was filled by the caller (stream_schedule); else K equal segments
};

// Number of tiles a device-resident MSM is cut into (1 = one pass over all points); see plan_stream_train.  Measured
// (profiles/r02_tiles.txt): G1 from 2^22 points on in tiles of 2^21 (235 MB of points), G2 from 2^23 on in tiles of 2^20
// (also 235 MB); at most MLHIP_MAX_SEGMENTS tiles.
// MLHIP_TILE_LOG2 = t forces tiles of 2^t points for every n above that (0 = never tile).
// (can_stream: the plan has the auxiliary stream and the carry-free copy; edwards: plan_use_edwards)
inline int resident_tiles(bool can_stream, bool kG2, int fold, size_t fold_tile, bool edwards, size_t n) {
  if (!can_stream) return 1;
  if (fold) {  // one pass per tile of the table (an entry index addresses the rows of one tile)
    const size_t k = (n + fold_tile - 1) / fold_tile;
    return k < 2 ? 1 : (int)std::min<size_t>(k, MLHIP_MAX_SEGMENTS);
  }
  int lg = kG2 ? 20 : 21;
  size_t from = (size_t)1 << (kG2 ? 23 : 22);
  if (edwards) {  // 168-byte Niels triples: 2^20 of them are what 2^21 Weierstrass points weigh
    lg = 20;
    from = (size_t)1 << 21;
  }
  if (const char* e = getenv("MLHIP_TILE_LOG2")) {
    const int v = atoi(e);
    if (v <= 0) return 1;
    lg = v > 30 ? 30 : v;
    from = ((size_t)1 << lg) + 1;
  }
  if (n < from) return 1;
  size_t k = (n + ((size_t)1 << lg) - 1) >> lg;
  if (k > MLHIP_MAX_SEGMENTS) k = MLHIP_MAX_SEGMENTS;
  return k < 2 ? 1 : (int)k;
}

// Number of segments a host-buffer MSM is streamed in (1 = one upload, one pass).  Measured on MI355X / PCIe gen5
// (tools/perf_hostapi.py): from 2^19 points the transfer is worth hiding; MLHIP_STREAM_SEGMENTS overrides (0/1 = off).
inline int stream_segments(bool can_stream, bool kG1, size_t n) {
  // G1 and G2 stream through the carry-free kernels and their bucket state (always there unless MLHIP_ACC32=1, which runs
  // one pass) -- the condition stream_begin checks
  if (!can_stream) return 1;
  if (getenv("MLHIP_STREAM_SCHEDULE")) return n >= 2 ? 2 : 1;  // explicit segment weights (stream_schedule), any n
  if (const char* e = getenv("MLHIP_STREAM_SEGMENTS")) {
    int v = atoi(e);
    if (v < 2) return 1;
    if (v > MLHIP_MAX_SEGMENTS) v = MLHIP_MAX_SEGMENTS;
    return n >= (size_t)v ? v : 1;
  }
  // segments of 2^18 pairs: at 2^20 the call drops from 5.9 to 4.5 ms, at 2^22 from 21.9 to 12.8 ms (the device-only time)
  // G2 (BLS12-381): segments of 2^17 pairs, 14.9 -> 11.4 ms at 2^20.  For G1 from 2^20 pairs on the count returned here only
  // says "stream": the train replaces the equal segments by a growing schedule (stream_schedule, round 4)
  const size_t k = n >> (kG1 ? 18 : 17);
  return k < 2 ? 1 : (k > MLHIP_MAX_SEGMENTS ? MLHIP_MAX_SEGMENTS : (int)k);
}

// Number of tiles of the G1 + G2 MSM of one scalar vector (api_msm.hip: plan_shared)
inline int shared_segments(bool scalars_travel, size_t n) {
  int K = 1;
  if (scalars_travel) {
    // uploads to hide: segments of 2^17 pairs, as a host-buffer G2 MSM (stream_segments)
    K = (int)std::min<size_t>(std::max<size_t>(n >> 17, 1), MLHIP_MAX_SEGMENTS);
    if (const char* e = getenv("MLHIP_STREAM_SEGMENTS")) {
      const int v = atoi(e);
      K = v < 2 ? 1 : (int)std::min<size_t>(std::min<size_t>((size_t)v, n), MLHIP_MAX_SEGMENTS);
    }
  } else {
    // tiles of 2^20 pairs from 2^22 on (see resident_tiles: G1 gains from 2^22, G2 from 2^23, neither loses)
    if (n >= ((size_t)1 << 22)) K = (int)std::min<size_t>((n + ((size_t)1 << 20) - 1) >> 20, MLHIP_MAX_SEGMENTS);
    if (const char* e = getenv("MLHIP_TILE_LOG2")) {
      const int v = atoi(e);
      K = 1;
      if (v > 0 && v < 31 && n > ((size_t)1 << v)) K = (int)std::min<size_t>((n + ((size_t)1 << v) - 1) >> v, MLHIP_MAX_SEGMENTS);
    }
  }
  return K;
}

// Segment schedule of a host-buffer MSM (round 4; profiles/r04_hostapi.txt, same-box A/Bs at 2^20 pairs).  K equal
// segments expose the whole first upload and pay the per-segment costs (a sort train, one round trip of the bucket state,
// two pageable copies, shorter bucket lists) K times.  What bounds the call differs between the two host protocols:
//   (b) resident bases, only the 32-byte scalars travel -- a fifth of the kernels' time: TWO segments, 3 and 13 sixteenths of
//       the call; the second upload hides under the first segment's kernels and only one extra sort train is paid:
//       3.37 -> 3.23 ms against four equal segments, 0.02 ms above the resident MSM of the same box;
//   (c) points and scalars travel, 128 B a pair -- the copies (2.35 ms) run at about the kernels' rate (2.6 ms), so a later
//       segment may be at most ~1.1x the one before or the kernels wait for it, and every extra segment costs ~0.1 ms:
//       growing schedules LOSE (1,1,2,3,4,5: 4.28 ms; 2,3,5,6: 4.24; 1,2,2,3,4,4: 4.09) against four equal segments (3.99) --
//       equal segments of 2^18 pairs stay.  (What round 4 did gain for (c) is the split event: a segment's sort starts on
//       its scalars, under the upload of its points -- stream_tile.)
// MLHIP_STREAM_SCHEDULE="w0,w1,..." (weights, at most MLHIP_MAX_SEGMENTS) overrides; MLHIP_STREAM_SEGMENTS = K keeps K equal
// segments (what the tests use to force many segments on small inputs).
inline void stream_schedule(SegmentCuts& cx, bool points_travel, size_t tile, bool fold_tiles = false) {
  int w[MLHIP_MAX_SEGMENTS];
  int k = 0;
  if (const char* e = getenv("MLHIP_STREAM_SCHEDULE")) {
    for (const char* q = e; *q && k < MLHIP_MAX_SEGMENTS;) {
      const int v = atoi(q);
      if (v > 0) w[k++] = v;
      while (*q && *q != ',') q++;
      if (*q == ',') q++;
    }
  } else if (getenv("MLHIP_STREAM_SEGMENTS")) {
    return;  // K equal segments
  } else if (fold_tiles && cx.n > tile && !points_travel) {
    // a folded plan with several tiles: 3 x 2^16 pairs, the rest of the first tile, then the tiles (a segment cannot cross one)
    const size_t first = (size_t)3 << 16;
    int m = 0;
    cx.bound[0] = 0;
    if (tile > 2 * first) cx.bound[++m] = first;
    for (size_t t = tile; t < cx.n && m + 1 < MLHIP_MAX_SEGMENTS; t += tile) cx.bound[++m] = t;
    cx.bound[++m] = cx.n;
    cx.K = m;
    cx.scheduled = true;
    return;
  } else if (cx.n >= ((size_t)1 << 20) && !points_travel) {
    // resident bases: 3 x 2^16 pairs first, then segments that grow fourfold (the scalars of the next segment -- 0.6 ns a
    // pair on the wire -- must arrive within the kernels of this one -- 2.5 ns a pair) up to one tile (2^21 pairs: what keeps
    // a segment's W passes over its points near the chip, resident_tiles); a remainder shorter than the first segment joins
    // the segment before it.  2^20: 3 | 13 sixteenths; 2^21: 0.19 | 0.75 | 1.06 M; 2^22: 0.19 | 0.75 | 2.0 | 1.06 M.
    const size_t first = (size_t)3 << 16;
    size_t off = 0, len = first;
    int m = 0;
    cx.bound[0] = 0;
    while (off < cx.n && m < MLHIP_MAX_SEGMENTS) {
      size_t take = std::min(len, cx.n - off);
      if (cx.n - off - take < first || m + 1 == MLHIP_MAX_SEGMENTS) take = cx.n - off;  // no crumb at the end
      off += take;
      cx.bound[++m] = off;
      len = std::min(len * 4, tile);
    }
    if (m >= 2) {
      cx.K = m;
      cx.scheduled = true;
    }
    return;
  }
  if (k < 2) return;
  long long total = 0;
  for (int i = 0; i < k; i++) total += w[i];
  size_t cum = 0;
  int m = 0;
  cx.bound[0] = 0;
  for (int i = 0; i < k; i++) {
    cum += (size_t)w[i];
    size_t b = i + 1 == k ? cx.n : ((size_t)((unsigned __int128)cx.n * cum / (size_t)total) + 1023) / 1024 * 1024;
    if (b > cx.n) b = cx.n;
    if (b > cx.bound[m]) cx.bound[++m] = b;
  }
  if (m < 2) return;
  cx.K = m;
  cx.scheduled = true;
}
// the tile stream_schedule grows its segments up to: the tile of resident_tiles
inline size_t schedule_tile(int fold, size_t fold_tile, bool edwards) { return fold ? fold_tile : (size_t)1 << (edwards ? 20 : 21); }

// The cuts stream_begin fixes for its tiles: K equal segments unless the caller scheduled them, cut again at the tiles of a
// folded plan's table.  false: a folded plan with too many tiles (MLHIP_EINVAL).
inline bool segment_cuts(SegmentCuts& cx, int fold, size_t fold_tile) {
  if (!cx.scheduled) {
    const size_t seg = (cx.n + cx.K - 1) / cx.K;
    int k = 0;
    for (size_t off = 0; off < cx.n; off += seg) cx.bound[k++] = off;
    cx.bound[k] = cx.n;
    cx.K = k;
  }
  if (fold) {
    // no segment may cross a tile of the table: cut at the tile boundaries; if that makes too many segments, fall back to
    // the tiles themselves
    if ((cx.n + fold_tile - 1) / fold_tile > MLHIP_MAX_SEGMENTS) return false;
    size_t b[2 * MLHIP_MAX_SEGMENTS + 2];
    int m = 0;
    b[0] = 0;
    for (int s2 = 0; s2 < cx.K; s2++) {
      const size_t hi = cx.bound[s2 + 1];
      for (size_t t = (b[m] / fold_tile + 1) * fold_tile; t < hi; t += fold_tile) b[++m] = t;
      b[++m] = hi;
    }
    if (m > MLHIP_MAX_SEGMENTS) {
      m = 0;
      for (size_t t = fold_tile; t < cx.n; t += fold_tile) b[++m] = t;
      b[++m] = cx.n;
      if (m > MLHIP_MAX_SEGMENTS) return false;
    }
    for (int s2 = 0; s2 <= m; s2++) cx.bound[s2] = b[s2];
    cx.K = m;
  }
  cx.seg = 0;
  for (int s2 = 0; s2 < cx.K; s2++) cx.seg = std::max(cx.seg, cx.bound[s2 + 1] - cx.bound[s2]);
  return true;
}

}  // namespace mlhip
