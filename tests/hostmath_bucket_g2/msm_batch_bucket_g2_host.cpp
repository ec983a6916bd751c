// tests/hostmath_bucket_g2 -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the bucket route of the
// batched MSM (mathlib_amd/csrc/msm_batch_bucket.h) in its two newer uses, replayed on the CPU in the order the kernels run
// it: G2 (F = Fp2Field<C>, one lane here for a lane pair there: 6-bit windows, the 32 lanes of every (slice, window), ten
// lock-step reduction steps), and the indexed point load of the table-free path of mlhip_bases_msm_batch* (G1 and G2: a
// base-index list, or base0 + position).  The plan and the rows from msm_batch_bucket_plan / msm_batch_bucket_layout with the
// group's tuning; per slice the digit bytes lane by lane, msm_bucket_lane, msm_bucket_reduce_step, msm_bucket_combine; the other
// rows through msm_batch_chunk; the sum passes of msm_batch.h.  Driven by tests/test_msm_batch_bucket_g2_host.py.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../mathlib_amd/csrc/msm_batch_bucket.h"

using namespace mlhip;

// mode 0: points[first + j]; 1: points[index[first + j]]; 2: points[base0 + j]
template <class C, class F, int P>
static int batch(const void* points, size_t n_points, const uint32_t* index, int mode, const void* scalars, int mont,
                 const uint64_t* offsets, size_t k, long t_req, long s_req, int G, void* out, uint64_t* stats) {
  typedef MsmBucketShape<std::is_same<F, FpField<C>>::value> Shape;
  constexpr uint32_t LANES = Shape::BUCKETS;
  const int W = msm_win_layout(C::FR_BITS, Shape::WIDTH).W;
  const MsmBatchBucketPlan plan = msm_batch_bucket_plan(offsets, k, P, W, t_req, s_req, Shape::tuning());
  MsmBatchLayout L;
  std::vector<uint32_t> slices;
  if (!msm_batch_bucket_layout(L, slices, offsets, k, P, plan, G)) return -1;
  const Affine<F>* pts = (const Affine<F>*)points;
  const uint32_t* sc = (const uint32_t*)scalars;
  const MsmBucketIndexed indexed = {mode == 1 ? index : nullptr};
  auto at = [&](const MsmBatchChunk& ch, uint32_t j) -> size_t {
    const size_t a = mode == 0 ? MsmBucketDirect()(ch, j) : indexed(ch, j);
    if (a >= n_points) abort();
    return a;
  };
  const uint32_t row_bytes = msm_bucket_pad16(plan.S);
  std::vector<XYZZ<F>> cur(L.chunks.size()), next;
  std::vector<uint8_t> written(L.chunks.size(), 0);
  uint64_t largest = 0;
  // the bucket kernels: the rows listed as slices
  std::vector<uint8_t> digits;
  std::vector<XYZZ<F>> wsum(W);
  for (size_t i = 0; i < slices.size(); i++) {
    const MsmBatchChunk ch = L.chunks[slices[i]];
    if (ch.count <= (uint32_t)P || ch.count > plan.S) return -2;
    const uint32_t n16 = msm_bucket_pad16(ch.count);
    digits.assign(msm_bucket_digit_stride(plan.S, W), 0xff);  // what the digit lanes do not write must not be read
    for (uint32_t j = 0; j < n16; j++)
      msm_bucket_digits<C, Shape::WIDTH>(digits.data(), row_bytes, j, ch.count, sc + 8 * ch.first, mont != 0);
    for (int w = 0; w < W; w++)
      for (uint32_t j = 0; j < n16; j++) {
        const uint32_t mag = digits[(size_t)w * row_bytes + j] >> 1;
        if (mag > LANES) return -9;  // no lane (pair) owns such a bucket
        largest = mag > largest ? mag : largest;
      }
    for (int w = 0; w < W; w++) {
      XYZZ<F> v[LANES], old[LANES];
      for (uint32_t lane = 0; lane < LANES; lane++)
        msm_bucket_lane<F>(v[lane], digits.data() + (size_t)w * row_bytes, n16, lane, [&](Affine<F>& p, uint32_t j) {
          if (j >= ch.count) abort();  // a padding byte matched
          p = pts[at(ch, j)];
        });
      for (int step = 0; step < Shape::STEPS; step++) {
        memcpy(old, v, sizeof(v));
        for (uint32_t lane = 0; lane < LANES; lane++)
          msm_bucket_reduce_step<F, MsmBatchOps<F>, Shape::LOG>(v[lane], step, [&](XYZZ<F>& q, const XYZZ<F>&, uint32_t d) {
            if (lane + d < LANES)
              q = old[lane + d];
            else
              xyzz_set_inf<F>(q);
          });
      }
      wsum[w] = v[0];
    }
    msm_bucket_combine<F, MsmBatchOps<F>, Shape::WIDTH>(cur[slices[i]], C::FR_BITS, [&](XYZZ<F>& q, int w) { q = wsum[w]; });
    written[slices[i]]++;
  }
  // the Straus kernel: every row, skipping the slices
  for (size_t c = 0; c < L.chunks.size(); c++) {
    const MsmBatchChunk ch = L.chunks[c];
    if (ch.count < 1) return -3;
    if (ch.count > (uint32_t)P) continue;
    msm_batch_chunk<F, P, MsmBatchOps<F>>(cur[c], sc + 8 * ch.first, ch.count, mont != 0,
                                          [&](Affine<F>& p, int j) { p = pts[at(ch, (uint32_t)j)]; });
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
    stats[5] = largest;
  }
  return 0;
}

template <class C, class F>
static int batch_p(int P, const void* points, size_t n_points, const uint32_t* index, int mode, const void* scalars, int mont,
                   const uint64_t* offsets, size_t k, long t_req, long s_req, int G, void* out, uint64_t* stats) {
  switch (P) {
    case 1: return batch<C, F, 1>(points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 2: return batch<C, F, 2>(points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 4: return batch<C, F, 4>(points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 8: return batch<C, F, 8>(points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    default: return -7;
  }
}

template <class C>
static int batch_g(int group, int P, const void* points, size_t n_points, const uint32_t* index, int mode, const void* scalars,
                   int mont, const uint64_t* offsets, size_t k, long t_req, long s_req, int G, void* out, uint64_t* stats) {
  if (group == 1)
    return batch_p<C, FpField<C>>(P, points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
  return batch_p<C, Fp2Field<C>>(P, points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
}

template <bool G1>
static int layout_check(int fr_bits, int P, long t_req, long s_req, const uint64_t* offsets, size_t k, uint64_t* info) {
  typedef MsmBucketShape<G1> Shape;
  const int W = msm_win_layout(fr_bits, Shape::WIDTH).W;
  const MsmBatchBucketPlan plan = msm_batch_bucket_plan(offsets, k, P, W, t_req, s_req, Shape::tuning());
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

extern "C" {
// out[s] = the affine sum of segment s in the group (1 or 2); the points of pair i are points[i] (mode 0), points[index[i]]
// (mode 1) or points[position of i in its segment] (mode 2), every read below n_points; t_req / s_req as
// MLHIP_MSM_BATCH_BUCKET_MIN / _SLICE (-1: unset); stats = {rows, slices, T, S, passes, largest magnitude} (may be null).
int hbk2_msm_batch(int curve, int group, int P, const void* points, size_t n_points, const uint32_t* index, int mode,
                   const void* scalars, int mont, const uint64_t* offsets, size_t k, long t_req, long s_req, int G, void* out,
                   uint64_t* stats) {
  if (group != 1 && group != 2) return -8;
  switch (curve) {
    case 0: return batch_g<Bn254>(group, P, points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 1: return batch_g<Bls381>(group, P, points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    case 2: return batch_g<Bls377>(group, P, points, n_points, index, mode, scalars, mont, offsets, k, t_req, s_req, G, out, stats);
    default: return -8;
  }
}

// The plan and the rows of a call of the group, checked as tests/hostmath_bucket's hbk_layout_check does for G1 (rows
// contiguous and covering; Straus rows below T, slices from T on; the slice list exactly the rows with count > P; an
// all-short call equal to msm_batch_layout byte for byte).  info = {rows, slices, T, S, windows}
int hbk2_layout_check(int fr_bits, int group, int P, long t_req, long s_req, const uint64_t* offsets, size_t k, uint64_t* info) {
  return group == 1 ? layout_check<true>(fr_bits, P, t_req, s_req, offsets, k, info)
                    : layout_check<false>(fr_bits, P, t_req, s_req, offsets, k, info);
}

// {MIN default, SLICE_MIN, SLICE_MAX, waves, width, buckets, reduction steps} of the group
int hbk2_constants(int group, uint64_t* v) {
  const MsmBatchBucketTuning t = group == 1 ? MsmBucketShape<true>::tuning() : MsmBucketShape<false>::tuning();
  v[0] = t.min_default;
  v[1] = t.slice_min;
  v[2] = t.slice_max;
  v[3] = t.waves;
  v[4] = group == 1 ? MsmBucketShape<true>::WIDTH : MsmBucketShape<false>::WIDTH;
  v[5] = group == 1 ? MsmBucketShape<true>::BUCKETS : MsmBucketShape<false>::BUCKETS;
  v[6] = group == 1 ? MsmBucketShape<true>::STEPS : MsmBucketShape<false>::STEPS;
  return 0;
}
}
