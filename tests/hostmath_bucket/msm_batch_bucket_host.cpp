// tests/hostmath_bucket -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the bucket route of the
// batched MSM (mathlib_amd/csrc/msm_batch_bucket.h), replayed on the CPU in the order the kernels run it: the plan and the
// rows from msm_batch_bucket_plan / msm_batch_bucket_layout; per slice the digit bytes lane by lane, per (slice, window) the
// 64 lanes of msm_bucket_lane and the twelve lock-step reduction steps over the lanes' values, then msm_bucket_combine; the
// other rows through msm_batch_chunk; the sum passes of msm_batch.h.  G1.  Driven by tests/test_msm_batch_bucket_host.py.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_batch_bucket.h"

using namespace mlhip;

template <class C, int P>
static int batch(const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, long t_req, long s_req,
                 int G, void* out, uint64_t* stats) {
  typedef FpField<C> F;
  const int W = msm_win_layout(C::FR_BITS, MSM_BATCH_BUCKET_C).W;
  const MsmBatchBucketPlan plan = msm_batch_bucket_plan(offsets, k, P, W, t_req, s_req);
  MsmBatchLayout L;
  std::vector<uint32_t> slices;
  if (!msm_batch_bucket_layout(L, slices, offsets, k, P, plan, G)) return -1;
  const Affine<F>* pts = (const Affine<F>*)points;
  const uint32_t* sc = (const uint32_t*)scalars;
  const uint32_t row_bytes = msm_bucket_pad16(plan.S);
  std::vector<XYZZ<F>> cur(L.chunks.size()), next;
  std::vector<uint8_t> written(L.chunks.size(), 0);
  // the bucket kernels: the rows listed as slices
  std::vector<uint8_t> digits;
  std::vector<XYZZ<F>> wsum(W);
  for (size_t i = 0; i < slices.size(); i++) {
    const MsmBatchChunk ch = L.chunks[slices[i]];
    if (ch.count <= (uint32_t)P || ch.count > plan.S) return -2;
    const uint32_t n16 = msm_bucket_pad16(ch.count);
    digits.assign(msm_bucket_digit_stride(plan.S, W), 0xff);  // what the digit lanes do not write must not be read
    for (uint32_t j = 0; j < n16; j++) msm_bucket_digits<C>(digits.data(), row_bytes, j, ch.count, sc + 8 * ch.first, mont != 0);
    const Affine<F>* base = pts + ch.first;
    for (int w = 0; w < W; w++) {
      XYZZ<F> v[64], old[64];
      for (uint32_t lane = 0; lane < 64; lane++)
        msm_bucket_lane<F>(v[lane], digits.data() + (size_t)w * row_bytes, n16, lane, [&](Affine<F>& p, uint32_t j) {
          if (j >= ch.count) abort();  // a padding byte matched
          p = base[j];
        });
      for (int step = 0; step < MSM_BATCH_BUCKET_REDUCE_STEPS; step++) {
        memcpy(old, v, sizeof(v));
        for (uint32_t lane = 0; lane < 64; lane++)
          msm_bucket_reduce_step<F, MsmBatchOps<F>>(v[lane], step, [&](XYZZ<F>& q, const XYZZ<F>&, uint32_t d) {
            if (lane + d < 64)
              q = old[lane + d];
            else
              xyzz_set_inf<F>(q);
          });
      }
      wsum[w] = v[0];
    }
    msm_bucket_combine<F, MsmBatchOps<F>>(cur[slices[i]], C::FR_BITS, [&](XYZZ<F>& q, int w) { q = wsum[w]; });
    written[slices[i]]++;
  }
  // the Straus kernel: every row, skipping the slices
  for (size_t c = 0; c < L.chunks.size(); c++) {
    const MsmBatchChunk ch = L.chunks[c];
    if (ch.count < 1) return -3;
    if (ch.count > (uint32_t)P) continue;
    const Affine<F>* base = pts + ch.first;
    msm_batch_chunk<F, P, MsmBatchOps<F>>(cur[c], sc + 8 * ch.first, ch.count, mont != 0, [&](Affine<F>& p, int j) { p = base[j]; });
    written[c]++;
  }
  for (size_t c = 0; c < L.chunks.size(); c++)
    if (written[c] != 1) return -4;  // every row is written by exactly one kernel kind
  const size_t passes = L.pass_begin.size() - 1;
  for (size_t q = 0; q < passes; q++) {
    const size_t g0 = L.pass_begin[q], g1 = L.pass_begin[q + 1];
    const bool last = q + 1 == passes;
    if (last && g1 - g0 != k) return -5;
    next.assign(g1 - g0, XYZZ<F>());
    for (size_t g = g0; g < g1; g++) {
      const MsmBatchGroup gr = L.groups[g];
      if (gr.count > (uint32_t)G || (size_t)gr.begin + gr.count > cur.size()) return -6;
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
    stats[1] = slices.size();
    stats[2] = plan.T;
    stats[3] = plan.S;
    stats[4] = passes;
  }
  return 0;
}

template <class C>
static int batch_p(int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, long t_req,
                   long s_req, int G, void* out, uint64_t* stats) {
  switch (P) {
    case 1: return batch<C, 1>(points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 2: return batch<C, 2>(points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 4: return batch<C, 4>(points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 8: return batch<C, 8>(points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    default: return -7;
  }
}

extern "C" {
// out[s] = the affine sum of segment s (G1); t_req / s_req as MLHIP_MSM_BATCH_BUCKET_MIN / _SLICE (-1: unset);
// stats = {rows, slices, T, S, passes} (may be null).  0 on success.
int hbk_msm_batch(int curve, int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k,
                  long t_req, long s_req, int G, void* out, uint64_t* stats) {
  switch (curve) {
    case 0: return batch_p<Bn254>(P, points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 1: return batch_p<Bls381>(P, points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 2: return batch_p<Bls377>(P, points, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    default: return -8;
  }
}

// The plan and the rows of a call, checked: 0 when
//   * the rows of every segment are contiguous, in order, and cover its pairs exactly once (base0 = the position in it);
//   * a segment below T has rows of 1 .. P pairs, one of at least T rows of S pairs and a last one of 1 .. S;
//   * the slice list is exactly the rows with count > P, ascending: every row belongs to one kernel kind;
//   * with no segment of T pairs or more (or T = 0) the tables equal msm_batch_layout's byte for byte.
// info = {rows, slices, T, S, windows}
int hbk_layout_check(int fr_bits, int P, long t_req, long s_req, const uint64_t* offsets, size_t k, uint64_t* info) {
  const int W = msm_win_layout(fr_bits, MSM_BATCH_BUCKET_C).W;
  const MsmBatchBucketPlan plan = msm_batch_bucket_plan(offsets, k, P, W, t_req, s_req);
  MsmBatchLayout L, L0;
  std::vector<uint32_t> slices;
  if (!msm_batch_bucket_layout(L, slices, offsets, k, P, plan)) return -1;
  info[0] = L.chunks.size();
  info[1] = slices.size();
  info[2] = plan.T;
  info[3] = plan.S;
  info[4] = (uint64_t)W;
  if (plan.T && (plan.T < MSM_BATCH_BUCKET_MIN_FLOOR || plan.S <= (uint32_t)P)) return -2;
  size_t c = 0, sl = 0;
  bool any_long = false;
  for (size_t s = 0; s < k; s++) {
    const uint64_t a = offsets[s], b = offsets[s + 1];
    const bool is_long = plan.T && b - a >= plan.T;
    any_long |= is_long;
    const uint64_t len = is_long ? plan.S : (uint64_t)P;
    for (uint64_t f = a; f < b;) {
      if (c >= L.chunks.size()) return -3;
      const MsmBatchChunk ch = L.chunks[c];
      if (ch.first != f || ch.base0 != (uint32_t)(f - a)) return -4;
      const uint64_t want = b - f < len ? b - f : len;
      if (ch.count != want) return -5;
      const bool slice = ch.count > (uint32_t)P;
      if (slice && !is_long) return -6;
      if (slice) {
        if (sl >= slices.size() || slices[sl] != c) return -7;
        sl++;
      }
      f += ch.count;
      c++;
    }
  }
  if (c != L.chunks.size() || sl != slices.size()) return -8;
  if (!any_long) {
    if (!msm_batch_layout(L0, offsets, k, P)) return -9;
    if (!slices.empty() || L.chunks.size() != L0.chunks.size() || L.groups.size() != L0.groups.size() ||
        L.pass_begin != L0.pass_begin || L.max_mid != L0.max_mid)
      return -10;
    if (!L.chunks.empty() && memcmp(L.chunks.data(), L0.chunks.data(), L.chunks.size() * sizeof(MsmBatchChunk))) return -11;
    if (!L.groups.empty() && memcmp(L.groups.data(), L0.groups.data(), L.groups.size() * sizeof(MsmBatchGroup))) return -12;
  }
  return 0;
}

int hbk_constants(uint64_t* v) {
  v[0] = MSM_BATCH_BUCKET_MIN_DEFAULT;
  v[1] = MSM_BATCH_BUCKET_SLICE_MIN;
  v[2] = MSM_BATCH_BUCKET_SLICE_MAX;
  v[3] = MSM_BATCH_BUCKET_WAVES;
  return 0;
}
}
