/* mlhip_products.h -- K products of m pairs each, for any m, as six inline functions over the entry points of mlhip.h (see its
 * section "products of any length"): the length travels in the pairs_per_product / ppp argument of mlhip_miller_loop[_device],
 * mlhip_miller_loop_prepared[_device] and mlhip_pairing_prepared[_device] as MLHIP_PRODUCT_PAIRS(m), so the library's dynamic
 * symbol table stays what it was.  m <= 4 is the plain call.  C, C++ and cgo. */
#ifndef MLHIP_PRODUCTS_H
#define MLHIP_PRODUCTS_H

#include "mlhip.h"

/* out[k] = prod_{j < m} MillerLoop(g1[k m + j], g2[k m + j]) for k < n_products; not final-exponentiated */
static inline int mlhip_miller_loop_products(int curve_id, const void* g1, const void* g2, size_t m, size_t n_products,
                                             void* out_gt) {
  return mlhip_miller_loop(curve_id, g1, g2, MLHIP_PRODUCT_PAIRS(m), n_products, out_gt);
}
/* the same on device pointers, in order on `stream` */
static inline int mlhip_miller_loop_products_device(int curve_id, const void* d_g1, const void* d_g2, size_t m, size_t n_products,
                                                    void* d_out_gt, void* stream) {
  return mlhip_miller_loop_device(curve_id, d_g1, d_g2, MLHIP_PRODUCT_PAIRS(m), n_products, d_out_gt, stream);
}
/* out[k] = prod_{j < m} MillerLoop(g1[k m + j], Q[q_index ? q_index[j] : j]) against the handle's points; q_index: m host
 * entries (repeats allowed) or NULL, which needs m <= the handle's count */
static inline int mlhip_miller_loop_prepared_products(mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t m,
                                                      size_t n_products, void* out_gt) {
  return mlhip_miller_loop_prepared(h, g1, q_index, MLHIP_PRODUCT_PAIRS(m), n_products, out_gt);
}
static inline int mlhip_miller_loop_prepared_products_device(mlhip_g2_prepared* h, const void* d_g1, const uint32_t* q_index,
                                                             size_t m, size_t n_products, void* d_out_gt, void* stream) {
  return mlhip_miller_loop_prepared_device(h, d_g1, q_index, MLHIP_PRODUCT_PAIRS(m), n_products, d_out_gt, stream);
}
/* out[k] = FExp of the same product */
static inline int mlhip_pairing_prepared_products(mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t m,
                                                  size_t n_products, void* out_gt) {
  return mlhip_pairing_prepared(h, g1, q_index, MLHIP_PRODUCT_PAIRS(m), n_products, out_gt);
}
static inline int mlhip_pairing_prepared_products_device(mlhip_g2_prepared* h, const void* d_g1, const uint32_t* q_index,
                                                         size_t m, size_t n_products, void* d_out_gt, void* stream) {
  return mlhip_pairing_prepared_device(h, d_g1, q_index, MLHIP_PRODUCT_PAIRS(m), n_products, d_out_gt, stream);
}

#endif
