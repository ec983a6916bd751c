/* mlhip_subgroup.h -- batched Mul for points promised in G1 / G2 as two inline functions over the entry points of mlhip.h
 * (see its section "points promised in G1 / G2"): the promise travels in the group argument of mlhip_scalar_mul /
 * mlhip_scalar_mul_device as MLHIP_GROUP_SUBGROUP(group), so the library's dynamic symbol table stays what it was.
 * C, C++ and cgo. */
#ifndef MLHIP_SUBGROUP_H
#define MLHIP_SUBGROUP_H

#include "mlhip.h"

/* out[i] = [scalars[i]] points[i * point_stride] for points in the prime-order subgroup (or at infinity); group =
 * MLHIP_GROUP_G1 / _G2, anything else is MLHIP_EINVAL */
static inline int mlhip_scalar_mul_subgroup(int curve_id, int group, const void* points, size_t point_stride,
                                            const void* scalars, int scalars_mont, size_t n, void* out_affine) {
  return mlhip_scalar_mul(curve_id, MLHIP_GROUP_SUBGROUP(group), points, point_stride, scalars, scalars_mont, n, out_affine);
}
/* the same on device pointers, asynchronous and in order on `stream` */
static inline int mlhip_scalar_mul_subgroup_device(int curve_id, int group, const void* d_points, size_t point_stride,
                                                   const void* d_scalars, int scalars_mont, size_t n, void* d_out_affine,
                                                   void* stream) {
  return mlhip_scalar_mul_device(curve_id, MLHIP_GROUP_SUBGROUP(group), d_points, point_stride, d_scalars, scalars_mont, n,
                                 d_out_affine, stream);
}

#endif
