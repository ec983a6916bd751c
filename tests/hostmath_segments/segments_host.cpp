// tests/hostmath_segments -- g++ build of mathlib_amd/csrc/msm_segments.h (no HIP): how an MSM is cut into segments and
// tiles, called through ctypes by tests/test_msm_segments_host.py.  The MLHIP_* switches are read from the environment per
// call, as in the library.
#include "../../mathlib_amd/csrc/msm_segments.h"

using namespace mlhip;

extern "C" {

int hseg_max_segments() { return MLHIP_MAX_SEGMENTS; }

int hseg_resident_tiles(int can_stream, int g2, int fold, size_t fold_tile, int edwards, size_t n) {
  return resident_tiles(can_stream != 0, g2 != 0, fold, fold_tile, edwards != 0, n);
}

int hseg_stream_segments(int can_stream, int g1, size_t n) { return stream_segments(can_stream != 0, g1 != 0, n); }

int hseg_shared_segments(int scalars_travel, size_t n) { return shared_segments(scalars_travel != 0, n); }

// The cuts of one train of K >= min_K segments, as plan_stream_train with `schedule` (shared == 0: a G1 MSM whose scalars travel is
// scheduled first) or without (shared != 0: the G1 + G2 pair) followed by stream_begin make them.  bound: MLHIP_MAX_SEGMENTS + 1 entries.
// 0, or 1 = "bad segment count", 2 = "folded plan: too many tiles" (both MLHIP_EINVAL in the library).
int hseg_train(int g1, size_t n, int K, int min_K, int fold, size_t fold_tile, int scalars_travel, int points_travel, int edwards,
               int shared, size_t* bound, int* K_out, size_t* seg_out) {
  SegmentCuts cx;
  cx.n = n;
  cx.K = K;
  if (!shared && scalars_travel && g1) stream_schedule(cx, points_travel != 0, schedule_tile(fold, fold_tile, edwards != 0), fold != 0);
  if (cx.n == 0 || cx.K < min_K || cx.K > MLHIP_MAX_SEGMENTS) return 1;
  if (!segment_cuts(cx, fold, fold_tile)) return 2;
  for (int s = 0; s <= cx.K; s++) bound[s] = cx.bound[s];
  *K_out = cx.K;
  *seg_out = cx.seg;
  return 0;
}
}
