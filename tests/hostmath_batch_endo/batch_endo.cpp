// TEST ARTIFACT -- host (g++, -DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) build of the two per-lane bodies of
// mathlib_amd/csrc/msm_batch_endo.h, the Straus chunks of mlhip_msm_batch* for points promised in G1 / G2, replayed lane by
// lane in the order the kernels run them: chunk table and sum passes from msm_batch_layout, the split body per chunk,
// msm_batch_sum per group, xyzz_to_affine in the last pass (tests/hostmath_batch with the chunk body exchanged).  G2 runs
// the body over one-lane Fp2 (the kernel uses lane pairs).  Loaded by tests/test_msm_batch_subgroup_host.py through ctypes;
// it is NOT part of libmlhip.so.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_batch_endo.h"

using namespace mlhip;

// -3: no split for this (curve, group); -5: P is not compiled for this group
template <class C, class F, int P>
static int batch(const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, void* out) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  if constexpr (!ScalarMulEndo<C, kG1>::AVAILABLE) {
    return -3;
  } else if constexpr (!msm_batch_endo_p_compiled<kG1>(P)) {
    return -5;
  } else {
    MsmBatchLayout L;
    if (!msm_batch_layout(L, offsets, k, P)) return -1;
    const Affine<F>* pts = (const Affine<F>*)points;
    const uint32_t* sc = (const uint32_t*)scalars;
    std::vector<XYZZ<F>> cur(L.chunks.size()), next;
    for (size_t c = 0; c < L.chunks.size(); c++) {
      const MsmBatchChunk ch = L.chunks[c];
      if (ch.count < 1 || ch.count > (uint32_t)P) return -2;
      const Affine<F>* base = pts + ch.first;
      auto load = [&](Affine<F>& p, int j) { p = base[j]; };
      if constexpr (kG1)
        msm_batch_chunk_endo_g1<F, P, MsmBatchOps<F>>(cur[c], sc + 8 * ch.first, ch.count, mont != 0, load);
      else
        msm_batch_chunk_endo_g2<F, P, MsmBatchOps<F>>(cur[c], sc + 8 * ch.first, ch.count, mont != 0, load);
    }
    const size_t passes = L.pass_begin.size() - 1;
    for (size_t q = 0; q < passes; q++) {
      const size_t g0 = L.pass_begin[q], g1 = L.pass_begin[q + 1];
      next.assign(g1 - g0, XYZZ<F>());
      for (size_t g = g0; g < g1; g++) {
        const MsmBatchGroup gr = L.groups[g];
        msm_batch_sum<F, MsmBatchOps<F>>(next[g - g0], gr.count, [&](XYZZ<F>& p, uint32_t i) { p = cur[gr.begin + i]; });
      }
      if (q + 1 == passes) {
        if (g1 - g0 != k) return -4;
        Affine<F>* o = (Affine<F>*)out;
        for (size_t s = 0; s < k; s++) xyzz_to_affine<F>(o[s], next[s]);
      }
      cur.swap(next);
    }
    return 0;
  }
}

template <class C, class F>
static int batch_p(int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, void* out) {
  switch (P) {
    case 1: return batch<C, F, 1>(points, scalars, mont, offsets, k, out);
    case 2: return batch<C, F, 2>(points, scalars, mont, offsets, k, out);
    case 4: return batch<C, F, 4>(points, scalars, mont, offsets, k, out);
    case 8: return batch<C, F, 8>(points, scalars, mont, offsets, k, out);
    default: return -5;
  }
}

template <class C>
static int batch_group(int group, int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k,
                       void* out) {
  if (group == 1) return batch_p<C, FpField<C>>(P, points, scalars, mont, offsets, k, out);
  if (group == 2) return batch_p<C, Fp2Field<C>>(P, points, scalars, mont, offsets, k, out);
  return -6;
}

extern "C" {
// out[s] = the affine sum of segment s by the split chunks of length P.  0 on success.
int hbe_msm_batch(int curve, int group, int P, const void* points, const void* scalars, int mont, const uint64_t* offsets,
                  size_t k, void* out) {
  switch (curve) {
    case 0: return batch_group<Bn254>(group, P, points, scalars, mont, offsets, k, out);
    case 1: return batch_group<Bls381>(group, P, points, scalars, mont, offsets, k, out);
    case 2: return batch_group<Bls377>(group, P, points, scalars, mont, offsets, k, out);
    default: return -6;
  }
}
}
