// tests/hostmath_set -- g++ build of mathlib_amd/csrc/msm_set.h (no HIP): which members of a set of resident-bases handles
// share a sort train, how many tiles a class is cut into and when a set call shares at all, called through ctypes by
// tests/test_bases_set_host.py.  The MLHIP_* switches are read from the environment per call, as in the library.
#include "../../mathlib_amd/csrc/msm_set.h"

using namespace mlhip;

extern "C" {

int hset_max_members() { return MLHIP_SET_MAX_MEMBERS; }

// geo: k rows of 8 values (fold, c, Wd, fold_tile, W, M, bits, can_train); cls: k entries; returns the number of classes
int hset_classes(const long long* geo, int k, int* cls) {
  SetGeometry g[16];
  for (int i = 0; i < k && i < 16; i++) {
    const long long* r = geo + 8 * i;
    g[i].fold = (int)r[0];
    g[i].c = (int)r[1];
    g[i].Wd = (int)r[2];
    g[i].fold_tile = (size_t)r[3];
    g[i].W = (int)r[4];
    g[i].M = (uint32_t)r[5];
    g[i].bits = (int)r[6];
    g[i].can_train = r[7] != 0;
  }
  return set_classes(g, k, cls);
}

int hset_class_tiles(int fold, size_t fold_tile, int first_is_g1, int scalars_travel, size_t n) {
  SetGeometry g;
  g.fold = fold;
  g.fold_tile = fold_tile;
  return set_class_tiles(g, first_is_g1 != 0, scalars_travel != 0, n);
}

int hset_share(size_t n, int device_scalars) { return set_share(n, device_scalars != 0) ? 1 : 0; }
long long hset_share_min_n(int device_scalars) { return device_scalars ? MLHIP_SET_SHARE_MIN_N_DEVICE : MLHIP_SET_SHARE_MIN_N_HOST; }
}
