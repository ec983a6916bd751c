/* mlhip_bits.h -- short-scalar MSMs as three inline functions over the entry points of mlhip.h (see its section "short
 * scalars"): the scalar width travels in the window_c argument of mlhip_msm_plan_create / mlhip_msm_g1 / mlhip_msm_g2 as
 * MLHIP_WINDOW_BITS(window_c, scalar_bits), so the library's dynamic symbol table stays what it was.  C, C++ and cgo. */
#ifndef MLHIP_BITS_H
#define MLHIP_BITS_H

#include "mlhip.h"

/* A plan for scalars known to be below 2^scalar_bits. */
static inline int mlhip_msm_plan_create_bits(int curve_id, int group, size_t max_n, int window_c, int scalar_bits,
                                             mlhip_msm_plan** plan) {
  return mlhip_msm_plan_create(curve_id, group, max_n, MLHIP_WINDOW_BITS(window_c, scalar_bits), plan);
}
/* the width the plan was made for (fr_bits for a full-width plan) */
static inline int mlhip_msm_plan_scalar_bits(mlhip_msm_plan* plan, int* scalar_bits) {
  float v[12];
  int k;
  if (!scalar_bits) plan = 0; /* (a null plan is the library's MLHIP_EINVAL) */
  k = mlhip_msm_plan_timings(plan, v, 12);
  if (k < 0) return k;
  if (k < 12) return MLHIP_EINVAL;
  *scalar_bits = (int)v[11];
  return 0;
}
/* host-buffer form: mlhip_msm_g1 / mlhip_msm_g2 for short scalars (group = MLHIP_GROUP_G1 / _G2) */
static inline int mlhip_msm_bits(int curve_id, int group, const void* points, const void* scalars, int scalars_mont,
                                 int scalar_bits, size_t n, int window_c, void* out_affine) {
  const int wc = MLHIP_WINDOW_BITS(window_c, scalar_bits);
  if (group == MLHIP_GROUP_G2) return mlhip_msm_g2(curve_id, points, scalars, scalars_mont, n, wc, out_affine);
  if (group != MLHIP_GROUP_G1) return MLHIP_EINVAL;
  return mlhip_msm_g1(curve_id, points, scalars, scalars_mont, n, wc, out_affine);
}

#endif
