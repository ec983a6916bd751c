/* tests/cpp/scalar_mul_subgroup_c.c -- include/mlhip_subgroup.h compiled as C: the two inline functions and the macro behind
 * plain C symbols that tests/cpp/scalar_mul_subgroup_test.cpp calls. */
#include "mlhip_subgroup.h"

int c_scalar_mul_subgroup(int curve_id, int group, const void* points, size_t point_stride, const void* scalars, int scalars_mont,
                          size_t n, void* out_affine) {
  return mlhip_scalar_mul_subgroup(curve_id, group, points, point_stride, scalars, scalars_mont, n, out_affine);
}
int c_scalar_mul_subgroup_device(int curve_id, int group, const void* d_points, size_t point_stride, const void* d_scalars,
                                 int scalars_mont, size_t n, void* d_out_affine, void* stream) {
  return mlhip_scalar_mul_subgroup_device(curve_id, group, d_points, point_stride, d_scalars, scalars_mont, n, d_out_affine, stream);
}
int c_group_subgroup(int group) { return MLHIP_GROUP_SUBGROUP(group); }
