/* mlhip_sum_batch.h -- K independent point sums in one call as inline functions over the batch entry points of mlhip.h (see its
 * section "K independent point sums in one call"): "every scalar is 1" travels in `scalars_mont` of mlhip_msm_batch /
 * mlhip_msm_batch_device / mlhip_bases_msm_batch / mlhip_bases_msm_batch_device as MLHIP_SCALARS_UNIT, with a NULL scalar array,
 * so the library's dynamic symbol table stays what it was.  C, C++ and cgo. */
#ifndef MLHIP_SUM_BATCH_H
#define MLHIP_SUM_BATCH_H

#include "mlhip.h"

/* out[k] = the sum of points[offsets[k] .. offsets[k + 1]) (the batched mlhip_g1_sum / mlhip_g2_sum); group = MLHIP_GROUP_G1 /
 * _G2; offsets: k + 1 host entries as for mlhip_msm_batch; an empty segment gives the point at infinity.  Any points of the
 * curve, in any order and multiplicity; a point off the curve gives an undefined result for its own segment only, never a
 * fault.  MLHIP_ENODEVICE without a device. */
static inline int mlhip_sum_batch(int curve_id, int group, const void* points, const uint64_t* offsets, size_t k,
                                  void* out_affine) {
  return mlhip_msm_batch(curve_id, group, points, NULL, MLHIP_SCALARS_UNIT, offsets, k, out_affine);
}
/* the same on device pointers (offsets in host memory), asynchronous and in order on `stream` */
static inline int mlhip_sum_batch_device(int curve_id, int group, const void* d_points, const uint64_t* offsets, size_t k,
                                         void* d_out_affine, void* stream) {
  return mlhip_msm_batch_device(curve_id, group, d_points, NULL, MLHIP_SCALARS_UNIT, offsets, k, d_out_affine, stream);
}

/* out[k] = the sum over segment k of B[idx(i)], idx(i) = base_index[i], or i - offsets[k] when base_index is NULL
 * (mlhip_bases_msm_batch's rules: index < the handle's n, a segment at most n long without an index list, no set, no sharded
 * handle).  The handle's batch tables are neither built nor read. */
static inline int mlhip_bases_sum_batch(mlhip_bases* bases, const uint32_t* base_index, const uint64_t* offsets, size_t k,
                                        void* out_affine) {
  return mlhip_bases_msm_batch(bases, NULL, MLHIP_SCALARS_UNIT, base_index, offsets, k, out_affine);
}
/* the same with the outputs written to device memory, in order on `stream` (base_index and offsets in host memory) */
static inline int mlhip_bases_sum_batch_device(mlhip_bases* bases, const uint32_t* base_index, const uint64_t* offsets, size_t k,
                                               void* stream, void* d_out_affine) {
  return mlhip_bases_msm_batch_device(bases, NULL, MLHIP_SCALARS_UNIT, base_index, offsets, k, stream, d_out_affine);
}

#endif
