// pairing_products.h -- K products of m pairs each, for any m (include/mlhip.h: MLHIP_PRODUCT_PAIRS):
// how a product is cut into the groups one Miller loop takes, and the schedule by which the groups' Fp12 values are folded
// into one value per product.  Plain integers only: the Miller kernels (pairing_kernels.h, pairing_prepared_kernels.h), the
// launcher (pairing_products_run.h) and the host tests (tests/hostmath_products) all read the layout from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MLHIP_PP_HD __host__ __device__ __forceinline__
#else
#define MLHIP_PP_HD inline
#endif

namespace mlhip {

// What a Miller kernel gets by value.  Product k is cut into g = ceil(m / per) groups of `per` pairs with a shorter tail;
// group i = k g + j starts at pair k m + j per and holds min(per, m - j per) pairs.  g = 1 is the plain call: group i is
// product i, m <= 4 pairs from i m.
struct MillerGroups {
  uint32_t m;    // pairs per product
  uint32_t g;    // groups per product
  uint32_t per;  // pairs per full group: 1, 2 or 4 (g = 1: m)
};

inline MillerGroups miller_groups_plain(size_t ppp) { return MillerGroups{(uint32_t)ppp, 1u, (uint32_t)ppp}; }
inline MillerGroups miller_groups(size_t m, size_t per) {
  return MillerGroups{(uint32_t)m, (uint32_t)((m + per - 1) / per), (uint32_t)per};
}

// group i: its first pair, its number of pairs, and the slot of its first pair inside its product (the prepared kernels
// look their G2 points up by slot).  With g > 1 a launch covers fewer than 2^32 groups (pairing_products_run.h cuts a call
// into slabs of at most 1 GiB of partials), so the division is a 32-bit one.
MLHIP_PP_HD void miller_group(const MillerGroups& mg, size_t i, size_t& first, int& count, uint32_t& slot) {
  if (mg.g == 1) {
    first = i * mg.m;
    count = (int)mg.m;
    slot = 0;
    return;
  }
  const uint32_t k = (uint32_t)i / mg.g, j = (uint32_t)i - k * mg.g;
  slot = j * mg.per;
  first = (size_t)k * mg.m + slot;
  const uint32_t left = mg.m - slot;
  count = (int)(left < mg.per ? left : mg.per);
}

struct MillerGroupAt {
  size_t first;
  int count;
  uint32_t slot;
  MLHIP_PP_HD MillerGroupAt(const MillerGroups& mg, size_t i) { miller_group(mg, i, first, count, slot); }
};

// ---- the fold: part[k g + j] *= part[k g + j + (cur - half)] for j < half = floor(cur / 2), all products in one pass, until
// one value per product is left (the upper-onto-lower fold of mlhip_pairing_product, strided by g).  The pass that leaves one
// value writes it to out[k].  A pass never reads what it writes: j + (cur - half) >= half.
struct FoldPass {
  uint32_t cur, half;
  bool last;  // writes out[k] instead of part[k g]
};
// pass number `p` of the fold of g values; false when the fold is over (g = 1 has no pass: the Miller kernel wrote out[k])
inline bool fold_pass(uint32_t g, int p, FoldPass& f) {
  uint32_t cur = g;
  for (int q = 0; cur > 1; q++) {
    const uint32_t half = cur / 2;
    if (q == p) {
      f.cur = cur;
      f.half = half;
      f.last = cur - half == 1;
      return true;
    }
    cur -= half;
  }
  return false;
}
// value v of a pass over K products (v < K half): the two operands and whether the product goes to out
MLHIP_PP_HD void fold_operands(uint32_t g, uint32_t cur, uint32_t half, size_t v, size_t& k, size_t& lo, size_t& hi) {
  k = v / half;
  const size_t j = v - k * half;
  lo = k * g + j;
  hi = lo + (cur - half);
}

// ---- the group size ----------------------------------------------------------------------------------------------------
// One pair per group while the K m pairs leave the chip under-filled (latency: every Miller loop then has the shortest chain,
// and the fold's log2(m) products are cheap beside it); four pairs share one accumulator's squarings from `threshold` pairs
// on (throughput).  forced: MLHIP_MILLER_GROUP = 1 | 2 | 4, anything else is ignored.
constexpr size_t MILLER_GROUP4_FROM = (size_t)1 << 17;  // mlhip_pairing_product's measured switch (api_pairing.hip)
inline size_t miller_group_pick(size_t pairs, const char* forced) {
  if (forced && (forced[0] == '1' || forced[0] == '2' || forced[0] == '4') && forced[1] == 0) return (size_t)(forced[0] - '0');
  return pairs >= MILLER_GROUP4_FROM ? 4 : 1;
}

// ---- scratch: [index copy | K_slab g partials]; a call whose partials exceed `cap` runs in slabs of products ---------------
constexpr size_t MILLER_PRODUCTS_SCRATCH_CAP = (size_t)1 << 30;
// products per slab; 0: the partials of ONE product do not fit (MLHIP_EINVAL)
inline size_t miller_products_slab(size_t K, uint32_t g, size_t gt_bytes, size_t index_bytes, size_t cap = MILLER_PRODUCTS_SCRATCH_CAP) {
  if (index_bytes >= cap) return 0;
  const size_t fit = (cap - index_bytes) / gt_bytes / g;
  return fit < K ? fit : K;
}

}  // namespace mlhip
