// The pairing and Gt operations of one curve (mlhip_internal.h: MLHIP_TU_OPS): tu_pairing_<curve>.hip defines MLHIP_TU_CURVE and
// includes this.
#include "pairing_kernels.h"
#include "pairing_prepared_kernels.h"
#include "pairing_products_run.h"
using namespace mlhip;
int MLHIP_TU_FN(pairing)(int what, const void* d_g1, const void* d_g2, size_t ppp, size_t n, const void* d_in,
                        void* d_out, hipStream_t st) {
  return pairing_device<MLHIP_TU_CURVE>(what, d_g1, d_g2, ppp, n, d_in, d_out, st);
}
int MLHIP_TU_FN(fp_mul)(const void* d_a, const void* d_b, size_t n, int repeat, void* d_out, hipStream_t st) {
  return fp_mul_device<MLHIP_TU_CURVE>(d_a, d_b, n, repeat, d_out, st);
}
int MLHIP_TU_FN(gt_mul)(const void* d_a, const void* d_b, size_t n, void* d_out, hipStream_t st) {
  return gt_mul_device<MLHIP_TU_CURVE>(d_a, d_b, n, d_out, st);
}
int MLHIP_TU_FN(gt_exp)(const void* d_in, const void* d_scalars, int mont, size_t n, void* d_out, hipStream_t st) {
  return gt_exp_device<MLHIP_TU_CURVE>(d_in, d_scalars, mont, n, d_out, st);
}
int MLHIP_TU_FN(gt_exp_cyclo)(const void* d_in, const void* d_scalars, int mont, size_t n, void* d_out, hipStream_t st) {
  return gt_exp_cyclo_device<MLHIP_TU_CURVE>(d_in, d_scalars, mont, n, d_out, st);
}
int MLHIP_TU_FN(gt_decode)(const void* d_wire, size_t n, int subgroup_check, void* d_out, void* d_status, hipStream_t st) {
  return gt_decode_device<MLHIP_TU_CURVE>(d_wire, n, subgroup_check, d_out, d_status, st);
}
int MLHIP_TU_FN(gt_encode)(const void* d_in, size_t n, void* d_wire, hipStream_t st) {
  return gt_encode_device<MLHIP_TU_CURVE>(d_in, n, d_wire, st);
}
int MLHIP_TU_FN(gt_is_member)(const void* d_in, size_t n, void* d_status, void* d_decoded, hipStream_t st) {
  return gt_is_member_device<MLHIP_TU_CURVE>(d_in, n, d_status, d_decoded, st);
}
int MLHIP_TU_FN(gt_inverse)(const void* d_in, size_t n, void* d_out, hipStream_t st) {
  return gt_inverse_device<MLHIP_TU_CURVE>(d_in, n, d_out, st);
}
int MLHIP_TU_FN(g2_prepared)(mlhip_g2_prepared_tables* t, int what, const void* d_g1, const uint32_t* q_index, size_t ppp,
                            size_t n, void* d_out, hipStream_t st) {
  if (what < 0) return g2_prepared_build<MLHIP_TU_CURVE>(t, st);
  return g2_prepared_run<MLHIP_TU_CURVE>(t, what, d_g1, q_index, ppp, n, d_out, st,
                                         [](int w, const void* a, const void* b, size_t p, size_t k, const void* in, void* o, hipStream_t s) {
                                           return pairing_device<MLHIP_TU_CURVE>(w, a, b, p, k, in, o, s);
                                         });
}
int MLHIP_TU_FN(miller_products)(const mlhip_g2_prepared_tables* t, int what, const void* d_g1, const void* d_g2,
                                const uint32_t* q_index, size_t m, size_t n, void* d_out, hipStream_t st) {
  if (what < 0) {
    miller_products_release();
    return 0;
  }
  return miller_products_run<MLHIP_TU_CURVE>(t, what, d_g1, d_g2, q_index, m, n, d_out, st);
}
