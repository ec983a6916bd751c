// The MSM operations of one curve (mlhip_internal.h: MLHIP_TU_OPS): tu_msm_<curve>.hip defines MLHIP_TU_CURVE and includes this.
#include "msm_kernels.h"
using namespace mlhip;
int MLHIP_TU_FN(plan_alloc)(mlhip_msm_plan* p) {
  return p->group == MLHIP_GROUP_G1 ? plan_alloc<FpField<MLHIP_TU_CURVE>>(p) : plan_alloc<Fp2Field<MLHIP_TU_CURVE>>(p);
}
int MLHIP_TU_FN(plan_launch)(mlhip_msm_plan* p, const void* d_points, const void* d_scalars, int mont, size_t n,
                            hipStream_t st) {
  if (p->group == MLHIP_GROUP_G1) return plan_launch<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(p, d_points, d_scalars, mont, n, st);
  return plan_launch<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(p, d_points, d_scalars, mont, n, st);
}
int MLHIP_TU_FN(plan_finish)(mlhip_msm_plan* p, void* out_affine, void* out_xyzz) {
  if (p->group == MLHIP_GROUP_G1) return plan_finish<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(p, out_affine, out_xyzz);
  return plan_finish<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(p, out_affine, out_xyzz);
}
int MLHIP_TU_FN(plan_train)(mlhip_msm_plan* const* plans, void* const* d_points, const void* const* h_points, int k,
                           void* d_scalars, const void* h_scalars, int mont, size_t n, int segments, bool schedule, hipStream_t st) {
  return plan_stream_train<MLHIP_TU_CURVE>(plans, d_points, h_points, k, d_scalars, h_scalars, mont, n, segments, schedule, st);
}
int MLHIP_TU_FN(scalar_mul)(int group, const void* d_points, size_t point_stride, const void* d_scalars, int mont,
                              size_t n, void* d_out, hipStream_t st, bool subgroup) {
  if (group == MLHIP_GROUP_G1)
    return scalar_mul_device<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(d_points, point_stride, d_scalars, mont, n, d_out, st, subgroup);
  return scalar_mul_device<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(d_points, point_stride, d_scalars, mont, n, d_out, st, subgroup);
}
int MLHIP_TU_FN(plan_fold_build)(mlhip_msm_plan* p, const void* d_points, size_t n, hipStream_t st) {
  if (p->group == MLHIP_GROUP_G1) return plan_fold_build<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(p, d_points, n, st);
  return plan_fold_build<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(p, d_points, n, st);
}
int MLHIP_TU_FN(msm_batch)(int group, const void* d_points, const void* d_scalars, int mont, const uint64_t* offsets, size_t k,
                          void* d_out, hipStream_t st, bool subgroup) {
  if (group == MLHIP_GROUP_G1) return msm_batch_route_device<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(d_points, d_scalars, mont, offsets, k, d_out, st, subgroup);
  return msm_batch_route_device<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(d_points, d_scalars, mont, offsets, k, d_out, st, subgroup);
}
int MLHIP_TU_FN(bases_batch)(int group, mlhip_bases_batch_tables* t, const void* d_pts, size_t n_bases, const void* d_scalars,
                             int mont, const uint32_t* base_index, const uint64_t* offsets, size_t k, size_t need, void* d_out,
                             hipStream_t st) {
  if (group == MLHIP_GROUP_G1)
    return bases_batch_device<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(t, d_pts, n_bases, d_scalars, mont, base_index, offsets, k, need, d_out, st);
  return bases_batch_device<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(t, d_pts, n_bases, d_scalars, mont, base_index, offsets, k, need, d_out, st);
}
int MLHIP_TU_FN(point_sum)(int group, const void* d_points, size_t n, void* d_out, hipStream_t st) {
  if (group == MLHIP_GROUP_G1) return point_sum_device<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(d_points, n, d_out, st);
  return point_sum_device<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(d_points, n, d_out, st);
}
int MLHIP_TU_FN(sum_batch)(int group, const void* d_points, bool bases, const uint32_t* base_index, const uint64_t* offsets,
                          size_t k, void* d_out, hipStream_t st) {
  if (group == MLHIP_GROUP_G1) return sum_batch_device<MLHIP_TU_CURVE, FpField<MLHIP_TU_CURVE>>(d_points, bases, base_index, offsets, k, d_out, st);
  return sum_batch_device<MLHIP_TU_CURVE, Fp2Field<MLHIP_TU_CURVE>>(d_points, bases, base_index, offsets, k, d_out, st);
}
void MLHIP_TU_FN(release_cache)(void) {
  fixed_base_release();
  msm_batch_release();
}
