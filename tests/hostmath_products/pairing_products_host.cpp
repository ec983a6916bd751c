// tests/hostmath_products -- g++ build of the layout of the long Miller-loop products (mathlib_amd/csrc/pairing_products.h:
// the groups of a product, the fold schedule, the group pick, the slabs) and of the MLHIP_PRODUCT_PAIRS macro of
// include/mlhip.h.  Driven by tests/test_pairing_products_host.py.
#include <stdint.h>

#include "../../include/mlhip_products.h"
#include "../../mathlib_amd/csrc/pairing_products.h"

using namespace mlhip;

extern "C" {

// group i of K x m at `per` pairs a group (per = 0: the plain call, g = 1): out = {first pair, count, slot, g}
int pp_group(uint32_t m, uint32_t per, uint64_t i, uint64_t* out) {
  const MillerGroups mg = per ? miller_groups(m, per) : miller_groups_plain(m);
  const MillerGroupAt at(mg, (size_t)i);
  out[0] = at.first;
  out[1] = (uint64_t)at.count;
  out[2] = at.slot;
  out[3] = mg.g;
  return 0;
}

// The fold of K products of g values replayed on words: part[k g + j] holds a residue modulo `mod`; every pass multiplies as
// k_gt_fold does (value v of K half, fold_operands), the last one into out[k].  Returns the number of passes; with g = 1
// nothing runs and out is left alone.  reads[i] counts how often part[i] was an operand.
int pp_fold(uint32_t g, uint64_t K, uint64_t mod, uint64_t* part, uint64_t* out, uint32_t* reads) {
  FoldPass f;
  int p = 0;
  for (; fold_pass(g, p, f); p++) {
    for (uint64_t v = 0; v < K * f.half; v++) {
      size_t k, lo, hi;
      fold_operands(g, f.cur, f.half, (size_t)v, k, lo, hi);
      reads[lo]++;
      reads[hi]++;
      const uint64_t r = (uint64_t)((unsigned __int128)part[lo] * part[hi] % mod);
      if (f.last)
        out[k] = r;
      else
        part[lo] = r;
    }
  }
  return p;
}

uint64_t pp_pick(uint64_t pairs, const char* forced) { return miller_group_pick((size_t)pairs, forced); }
uint64_t pp_slab(uint64_t K, uint32_t g, uint64_t gt_bytes, uint64_t index_bytes, uint64_t cap) {
  return miller_products_slab((size_t)K, g, (size_t)gt_bytes, (size_t)index_bytes, (size_t)cap);
}

// MLHIP_PRODUCT_PAIRS on a 64-bit, a signed and an unsigned 32-bit argument
uint64_t pp_pack_u64(uint64_t m) { return MLHIP_PRODUCT_PAIRS(m); }
uint64_t pp_pack_int(int m) { return MLHIP_PRODUCT_PAIRS(m); }
uint64_t pp_pack_u32(uint32_t m) { return MLHIP_PRODUCT_PAIRS(m); }
}
