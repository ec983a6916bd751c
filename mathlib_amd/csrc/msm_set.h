// msm_set.h -- the policy of a SET of resident-bases handles (include/mlhip.h: mlhip_bases_set_create): which members share
// one sort train per tile, how many tiles a class is cut into, and from which size sharing is the default.  Plain integer
// arithmetic without a HIP type, so that tests/hostmath_set replays it on the CPU (tests/test_bases_set_host.py).  The train
// that runs a class is plan_stream_train (msm_plan.h); api_bases.hip asks the functions below.
#pragma once
#include <cstddef>
#include <cstdint>

#include "msm_segments.h"

#define MLHIP_SET_MAX_MEMBERS 4

namespace mlhip {

// What the entry lists of a tile depend on besides the scalars: the geometry of the member's plan (mlhip_internal.h).  None
// of it names the group: a G1 member and a G2 member of equal geometry read the same lists.
//   can_train: the plan runs the segment train (the auxiliary stream and the carry-free copy: plan_can_stream) and sorts on
//   the two-level path, whose lists another plan's accumulation can read.
struct SetGeometry {
  int fold = 0, c = 0, Wd = 0;
  size_t fold_tile = 0;
  int W = 0;
  uint32_t M = 0;
  int bits = 0;
  bool can_train = false;
};

inline bool set_same_geometry(const SetGeometry& a, const SetGeometry& b) {
  return a.fold == b.fold && a.c == b.c && a.Wd == b.Wd && a.fold_tile == b.fold_tile && a.W == b.W && a.M == b.M && a.bits == b.bits;
}

// cls[i] = the class of member i, classes numbered in the order of their first member; returns the number of classes.
// Members of equal geometry that can run the train form one class (one sort per tile, one accumulation per member); a
// member that cannot is a class of its own and runs what its own handle would.
inline int set_classes(const SetGeometry* g, int k, int* cls) {
  int n_cls = 0;
  for (int i = 0; i < k; i++) {
    cls[i] = -1;
    if (g[i].can_train)
      for (int j = 0; j < i && cls[i] < 0; j++)
        if (g[j].can_train && set_same_geometry(g[i], g[j])) cls[i] = cls[j];
    if (cls[i] < 0) cls[i] = n_cls++;
  }
  return n_cls;
}

// Tiles of a class of two or more members over n scalars.
//   scalars_travel: the class uploads the call's host scalars (the first class of mlhip_bases_msm on a set) -- the segments of
//   the first member's own mlhip_bases_msm (stream_segments; a G1 first member's are then scheduled as a single plan's are);
//   otherwise the scalars are in device memory: the tiles of a folded plan's table, or those of the shared-scalar pair.
inline int set_class_tiles(const SetGeometry& g, bool first_is_g1, bool scalars_travel, size_t n) {
  if (scalars_travel) return stream_segments(true, first_is_g1, n);
  if (g.fold) return resident_tiles(true, false, g.fold, g.fold_tile, false, n);
  return shared_segments(false, n);
}

// Does a set call share (one upload, one sort train per class) or run every member's own MSM in turn?
//   MLHIP_BASES_SET_SHARE = 0: never (the second implementation: parity tests and the A/B); = 1: at every size;
//   unset: from the smallest size at which tools/perf_bases_set.py --ab measured the set call level with or ahead of the k
//   separate calls in every cell (profiles/bases_set_ab.txt; grid 2^12, 2^16, 2^20, 2^22):
//     host scalars    2^12 -- ahead in every measured cell (0.77 .. 0.996 of the separate calls); smaller calls were not measured
//     device scalars  2^16 -- at 2^12 the BLS12-381 cells were 1.0 % and 1.4 % BEHIND where two runs of the separate calls
//                     differed by 0.0 % and 0.2 %: a train of one tile always queues the long-bucket step and never takes the
//                     quad-lane kernel of a small one-pass MSM, and saves no upload; from 2^16 on every cell is ahead
#define MLHIP_SET_SHARE_MIN_N_HOST (1 << 12)
#define MLHIP_SET_SHARE_MIN_N_DEVICE (1 << 16)
inline bool set_share(size_t n, bool device_scalars) {
  if (const char* e = getenv("MLHIP_BASES_SET_SHARE")) {
    if (e[0] == '0') return false;
    if (e[0] == '1') return true;
  }
  return n >= (size_t)(device_scalars ? MLHIP_SET_SHARE_MIN_N_DEVICE : MLHIP_SET_SHARE_MIN_N_HOST);
}

}  // namespace mlhip
