/* mlhip_device_result.h -- device-result MSM plans and handles as inline functions over the entry points of mlhip.h (see
 * its section "device results"): the flavour travels in the window_c argument of mlhip_msm_plan_create / mlhip_bases_create
 * / mlhip_bases_create_device as MLHIP_WINDOW_DEVICE_RESULT, so the library's dynamic symbol table stays what it was.
 * C, C++ and cgo. */
#ifndef MLHIP_DEVICE_RESULT_H
#define MLHIP_DEVICE_RESULT_H

#include "mlhip.h"

/* A plan whose mlhip_msm_run / mlhip_msm_finish leave the result in device memory, in stream order, without a host wait.
 * scalar_bits as in mlhip_msm_plan_create_bits (0 = full width). */
static inline int mlhip_msm_plan_create_device_result(int curve_id, int group, size_t max_n, int window_c, int scalar_bits,
                                                      mlhip_msm_plan** plan) {
  return mlhip_msm_plan_create(curve_id, group, max_n, MLHIP_WINDOW_BITS(window_c, scalar_bits) | MLHIP_WINDOW_DEVICE_RESULT,
                               plan);
}
/* *on = 1 for a device-result plan, 0 for a host-result one */
static inline int mlhip_msm_plan_is_device_result(mlhip_msm_plan* plan, int* on) {
  float v[13];
  int k;
  if (!on) plan = 0; /* (a null plan is the library's MLHIP_EINVAL) */
  k = mlhip_msm_plan_timings(plan, v, 13);
  if (k < 0) return k;
  if (k < 13) return MLHIP_EINVAL;
  *on = v[12] != 0.0f;
  return 0;
}
/* mlhip_msm_run on a device-result plan: d_out_affine (and d_out_xyzz, or NULL) are device pointers on the plan's device,
 * written in order on `stream`; the call returns once everything is queued */
static inline int mlhip_msm_run_device(mlhip_msm_plan* plan, const void* d_points, const void* d_scalars, int scalars_mont,
                                       size_t n, void* stream, void* d_out_affine, void* d_out_xyzz) {
  int on = 0;
  int rc = mlhip_msm_plan_is_device_result(plan, &on);
  if (rc) return rc;
  if (!on) return MLHIP_EINVAL;
  return mlhip_msm_run(plan, d_points, d_scalars, scalars_mont, n, stream, d_out_affine, d_out_xyzz);
}
/* mlhip_msm_finish on a device-result plan, after mlhip_msm_launch / mlhip_msm_launch_shared: queues the tail and the
 * delivery on the stream of the pending launch and returns */
static inline int mlhip_msm_finish_device(mlhip_msm_plan* plan, void* d_out_affine, void* d_out_xyzz) {
  int on = 0;
  int rc = mlhip_msm_plan_is_device_result(plan, &on);
  if (rc) return rc;
  if (!on) return MLHIP_EINVAL;
  return mlhip_msm_finish(plan, d_out_affine, d_out_xyzz);
}
/* A device-result handle over n points in host memory (points_on_device = 0) or in the current device's memory (!= 0):
 * always one device */
static inline int mlhip_bases_create_device_result(int curve_id, int group, const void* points, int points_on_device, size_t n,
                                                   int window_c, mlhip_bases** bases) {
  const int wc = (window_c < 0 || window_c > 255 ? 0xFF : window_c) | MLHIP_WINDOW_DEVICE_RESULT;
  if (points_on_device) return mlhip_bases_create_device(curve_id, group, points, n, wc, bases);
  return mlhip_bases_create(curve_id, group, points, n, wc, bases);
}
/* mlhip_bases_msm_device on a device-result handle: d_out_affine is a device pointer, written in order on `stream` */
static inline int mlhip_bases_msm_to_device(mlhip_bases* bases, const void* d_scalars, int scalars_mont, size_t n, void* stream,
                                            void* d_out_affine) {
  int on = 0;
  int rc = mlhip_msm_plan_is_device_result(mlhip_bases_plan(bases), &on);
  if (rc) return rc;
  if (!on) return MLHIP_EINVAL;
  return mlhip_bases_msm_device(bases, d_scalars, scalars_mont, n, stream, d_out_affine);
}

#endif
