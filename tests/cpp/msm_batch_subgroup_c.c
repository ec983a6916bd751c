/* tests/cpp/msm_batch_subgroup_c.c -- include/mlhip_subgroup.h compiled as C: the two inline batched-MSM functions and the
 * macro behind plain C symbols that tests/cpp/msm_batch_subgroup_test.cpp calls. */
#include "mlhip_subgroup.h"

int c_msm_batch_subgroup(int curve_id, int group, const void* points, const void* scalars, int scalars_mont,
                         const uint64_t* offsets, size_t k, void* out_affine) {
  return mlhip_msm_batch_subgroup(curve_id, group, points, scalars, scalars_mont, offsets, k, out_affine);
}
int c_msm_batch_subgroup_device(int curve_id, int group, const void* d_points, const void* d_scalars, int scalars_mont,
                                const uint64_t* offsets, size_t k, void* d_out_affine, void* stream) {
  return mlhip_msm_batch_subgroup_device(curve_id, group, d_points, d_scalars, scalars_mont, offsets, k, d_out_affine, stream);
}
int c_curve_subgroup_points(int curve_id) { return MLHIP_CURVE_SUBGROUP_POINTS(curve_id); }
