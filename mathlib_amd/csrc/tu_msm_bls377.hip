// MSM kernels instantiated for Bls377 (G1 over Fp, G2 over Fp2).
#include "msm_kernels.h"
using namespace mlhip;
int mlhip_tu_plan_alloc_Bls377(mlhip_msm_plan* p) {
  return p->group == MLHIP_GROUP_G1 ? plan_alloc<FpField<Bls377>>(p) : plan_alloc<Fp2Field<Bls377>>(p);
}
int mlhip_tu_plan_launch_Bls377(mlhip_msm_plan* p, const void* d_points, const void* d_scalars, int mont, size_t n,
                            hipStream_t st) {
  if (p->group == MLHIP_GROUP_G1) return plan_launch<Bls377, FpField<Bls377>>(p, d_points, d_scalars, mont, n, st);
  return plan_launch<Bls377, Fp2Field<Bls377>>(p, d_points, d_scalars, mont, n, st);
}
int mlhip_tu_plan_finish_Bls377(mlhip_msm_plan* p, void* out_affine, void* out_xyzz) {
  if (p->group == MLHIP_GROUP_G1) return plan_finish<Bls377, FpField<Bls377>>(p, out_affine, out_xyzz);
  return plan_finish<Bls377, Fp2Field<Bls377>>(p, out_affine, out_xyzz);
}
int mlhip_tu_plan_stream_Bls377(mlhip_msm_plan* p, void* d_points, void* d_scalars, const void* h_points,
                            const void* h_scalars, int mont, size_t n, int segments, hipStream_t st) {
  if (p->group == MLHIP_GROUP_G1) return plan_stream<Bls377, FpField<Bls377>>(p, d_points, d_scalars, h_points, h_scalars, mont, n, segments, st);
  return plan_stream<Bls377, Fp2Field<Bls377>>(p, d_points, d_scalars, h_points, h_scalars, mont, n, segments, st);
}
int mlhip_tu_plan_shared_Bls377(mlhip_msm_plan* g1, mlhip_msm_plan* g2, void* d_points_g1, void* d_points_g2, void* d_scalars,
                            const void* h_points_g1, const void* h_points_g2, const void* h_scalars, int mont, size_t n,
                            hipStream_t st) {
  return plan_stream_shared<Bls377>(g1, g2, d_points_g1, d_points_g2, d_scalars, h_points_g1, h_points_g2, h_scalars, mont, n, st);
}
int mlhip_tu_scalar_mul_Bls377(int group, const void* d_points, size_t point_stride, const void* d_scalars, int mont,
                              size_t n, void* d_out, hipStream_t st) {
  if (group == MLHIP_GROUP_G1)
    return scalar_mul_device<Bls377, FpField<Bls377>>(d_points, point_stride, d_scalars, mont, n, d_out, st);
  return scalar_mul_device<Bls377, Fp2Field<Bls377>>(d_points, point_stride, d_scalars, mont, n, d_out, st);
}
int mlhip_tu_plan_fold_build_Bls377(mlhip_msm_plan* p, const void* d_points, size_t n, hipStream_t st) {
  if (p->group == MLHIP_GROUP_G1) return plan_fold_build<Bls377, FpField<Bls377>>(p, d_points, n, st);
  return plan_fold_build<Bls377, Fp2Field<Bls377>>(p, d_points, n, st);
}
int mlhip_tu_msm_batch_Bls377(int group, const void* d_points, const void* d_scalars, int mont, const uint64_t* offsets, size_t k,
                          void* d_out, hipStream_t st) {
  if (group == MLHIP_GROUP_G1) return msm_batch_device<Bls377, FpField<Bls377>>(d_points, d_scalars, mont, offsets, k, d_out, st);
  return msm_batch_device<Bls377, Fp2Field<Bls377>>(d_points, d_scalars, mont, offsets, k, d_out, st);
}
int mlhip_tu_bases_batch_Bls377(int group, mlhip_bases_batch_tables* t, const void* d_pts, size_t n_bases, const void* d_scalars,
                             int mont, const uint32_t* base_index, const uint64_t* offsets, size_t k, size_t need, void* d_out,
                             hipStream_t st) {
  if (group == MLHIP_GROUP_G1)
    return bases_batch_device<Bls377, FpField<Bls377>>(t, d_pts, n_bases, d_scalars, mont, base_index, offsets, k, need, d_out, st);
  return bases_batch_device<Bls377, Fp2Field<Bls377>>(t, d_pts, n_bases, d_scalars, mont, base_index, offsets, k, need, d_out, st);
}
void mlhip_tu_release_cache_Bls377(void) {
  fixed_base_release();
  msm_batch_release();
}
