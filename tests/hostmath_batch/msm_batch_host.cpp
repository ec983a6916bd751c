// tests/hostmath_batch -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the batched MSM's
// layout builder and per-lane bodies (mathlib_amd/csrc/msm_batch.h), replayed on the CPU lane by lane in the order the
// kernels run them: chunk table and sum passes from msm_batch_layout, msm_batch_chunk per chunk, msm_batch_sum per group,
// xyzz_to_affine in the last pass.  G2 runs the same bodies over one-lane Fp2 (the kernels use lane pairs).
// Driven by tests/test_msm_batch_host.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_batch.h"

using namespace mlhip;

template <class C, class F, int P>
static int batch(const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, int G, void* out,
                 uint64_t* stats) {
  MsmBatchLayout L;
  if (!msm_batch_layout(L, offsets, k, P, G)) return -1;
  const Affine<F>* pts = (const Affine<F>*)points;
  const uint32_t* sc = (const uint32_t*)scalars;
  std::vector<XYZZ<F>> cur(L.chunks.size()), next;
  for (size_t c = 0; c < L.chunks.size(); c++) {
    const MsmBatchChunk ch = L.chunks[c];
    if (ch.count < 1 || ch.count > (uint32_t)P) return -2;
    const Affine<F>* base = pts + ch.first;
    msm_batch_chunk<F, P, MsmBatchOps<F>>(cur[c], sc + 8 * ch.first, ch.count, mont != 0,
                                          [&](Affine<F>& p, int j) { p = base[j]; });
  }
  const size_t passes = L.pass_begin.size() - 1;
  uint64_t longest = 0;
  for (size_t q = 0; q < passes; q++) {
    const size_t g0 = L.pass_begin[q], g1 = L.pass_begin[q + 1];
    const bool last = q + 1 == passes;
    if (last && g1 - g0 != k) return -3;
    next.assign(g1 - g0, XYZZ<F>());
    for (size_t g = g0; g < g1; g++) {
      const MsmBatchGroup gr = L.groups[g];
      if (gr.count > (uint32_t)G || (size_t)gr.begin + gr.count > cur.size()) return -4;
      longest = gr.count > longest ? gr.count : longest;
      msm_batch_sum<F, MsmBatchOps<F>>(next[g - g0], gr.count, [&](XYZZ<F>& p, uint32_t i) { p = cur[gr.begin + i]; });
    }
    if (last) {
      Affine<F>* o = (Affine<F>*)out;
      for (size_t s = 0; s < k; s++) xyzz_to_affine<F>(o[s], next[s]);
    }
    cur.swap(next);
  }
  if (stats) {
    stats[0] = L.chunks.size();
    stats[1] = passes;
    stats[2] = longest;
  }
  return 0;
}

template <class C, class F>
static int batch_p(int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, int G, void* out,
                   uint64_t* stats) {
  switch (P) {
    case 1: return batch<C, F, 1>(points, scalars, mont, offsets, k, G, out, stats);
    case 2: return batch<C, F, 2>(points, scalars, mont, offsets, k, G, out, stats);
    case 4: return batch<C, F, 4>(points, scalars, mont, offsets, k, G, out, stats);
    case 8: return batch<C, F, 8>(points, scalars, mont, offsets, k, G, out, stats);
    default: return -5;
  }
}

template <class C>
static int batch_group(int group, int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k,
                       int G, void* out, uint64_t* stats) {
  if (group == 1) return batch_p<C, FpField<C>>(P, points, scalars, mont, offsets, k, G, out, stats);
  return batch_p<C, Fp2Field<C>>(P, points, scalars, mont, offsets, k, G, out, stats);
}

extern "C" {
// out[s] = the affine sum of segment s; stats = {chunks, passes, longest group} (may be null).  0 on success.
int hmb_msm_batch(int curve, int group, int P, const void* points, const void* scalars, int mont, const uint64_t* offsets,
                  size_t k, int G, void* out, uint64_t* stats) {
  switch (curve) {
    case 0: return batch_group<Bn254>(group, P, points, scalars, mont, offsets, k, G, out, stats);
    case 1: return batch_group<Bls381>(group, P, points, scalars, mont, offsets, k, G, out, stats);
    case 2: return batch_group<Bls377>(group, P, points, scalars, mont, offsets, k, G, out, stats);
    default: return -6;
  }
}
}
