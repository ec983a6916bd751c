// Wire-format codec kernels instantiated for Bls377.
#define MLHIP_TU_CURVE Bls377
#include "tu_codec.inc"
int mlhip_tu_g1_count_outside_subgroup_Bls377(const void* d_pts, size_t n, uint32_t* d_bad, hipStream_t st) {
  return g1_count_outside_subgroup_device<Bls377>(d_pts, n, d_bad, st);
}
