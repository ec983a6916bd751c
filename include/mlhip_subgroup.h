/* mlhip_subgroup.h -- batched Mul and batched MSMs for points promised in G1 / G2 as inline functions over the entry points
 * of mlhip.h (see its sections "points promised in G1 / G2" and "batched MSMs over points promised in G1 / G2"): the promise
 * travels in the group argument of mlhip_scalar_mul / mlhip_scalar_mul_device as MLHIP_GROUP_SUBGROUP(group) and in the curve
 * id of mlhip_msm_batch / mlhip_msm_batch_device as MLHIP_CURVE_SUBGROUP_POINTS(curve_id), so the library's dynamic symbol
 * table stays what it was.  C, C++ and cgo. */
#ifndef MLHIP_SUBGROUP_H
#define MLHIP_SUBGROUP_H

#include "mlhip.h"

/* out[i] = [scalars[i]] points[i * point_stride] for points in the prime-order subgroup (or at infinity); group =
 * MLHIP_GROUP_G1 / _G2, anything else is MLHIP_EINVAL.  BN254 G1: the lattice split s = k1 + k2 lambda runs; the promise holds
 * for every point of the curve, and a point off the curve gives an undefined result for its own product only, never a fault. */
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

/* out[k] = sum over segment k of [scalars[i]] points[i] (mlhip_msm_batch) for points in the prime-order subgroup (or at
 * infinity); curve_id = 0, 1 or 2, anything else is MLHIP_EINVAL.  BN254 G1: the chunks run the lattice split; the promise holds
 * for every point of the curve, and a point off the curve gives an undefined result for its own segment only, never a fault. */
static inline int mlhip_msm_batch_subgroup(int curve_id, int group, const void* points, const void* scalars, int scalars_mont,
                                           const uint64_t* offsets, size_t k, void* out_affine) {
  return mlhip_msm_batch(MLHIP_CURVE_SUBGROUP_POINTS(curve_id), group, points, scalars, scalars_mont, offsets, k, out_affine);
}
/* the same on device pointers (offsets in host memory), asynchronous and in order on `stream` */
static inline int mlhip_msm_batch_subgroup_device(int curve_id, int group, const void* d_points, const void* d_scalars,
                                                  int scalars_mont, const uint64_t* offsets, size_t k, void* d_out_affine,
                                                  void* stream) {
  return mlhip_msm_batch_device(MLHIP_CURVE_SUBGROUP_POINTS(curve_id), group, d_points, d_scalars, scalars_mont, offsets, k,
                                d_out_affine, stream);
}

#endif
