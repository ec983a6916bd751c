// msm_sum_batch.h -- K independent point sums in one call (mlhip_msm_batch* / mlhip_bases_msm_batch* with
// MLHIP_SCALARS_UNIT): out[k] = sum of the points of segment k, no scalars.  Part of msm_kernels.h (after point_sum.h); the
// slice layout, the choice of S and the three loads above the kernels are plain C++ / __host__ __device__, so
// tests/hostmath_sum_batch replays them on the CPU.  Layout, counted operations and measurements: DESIGN.md section 21.
//
//   slices     a segment [a, b) of m points is cut into c = ceil(m / S) slices; slice j reads a + j, a + j + c, a + j + 2 c, ...
//              below b, so neighbouring lanes read neighbouring rows (as in k_point_sum).  A slice is a chunk of
//              msm_batch_layout_by with chunk_len = S: first = a + j, count = its points (1 .. S), base0 = j (its first point's
//              position in the segment).  The stride c of every slice travels in the `extra` block of msm_batch_run, one
//              uint32 per slice, in front of the index list of a handle call.
//   pass 0     one lane (G1) or lane pair (G2) per slice runs point_sum_lane (point_sum.h) over its rows and writes one XYZZ
//              partial: 1 mixed addition per point.
//   sum passes msm_batch_run's, unchanged: groups of at most MSM_BATCH_GROUP partials, the last pass to affine.  No lane runs
//              a chain longer than max(S, MSM_BATCH_GROUP).
//   loads      SumLoadPoints: points[i]; SumLoadIndexed: bases[base_index[i]]; SumLoadSegment: bases[i - a].
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "point_sum.h"

namespace mlhip {

// the S of a call: a power of two; the default rule picks from [SUM_BATCH_S_MIN, SUM_BATCH_S_MAX], MLHIP_SUM_BATCH_SLICE any
// power of two up to SUM_BATCH_S_FORCE_MAX
constexpr uint32_t SUM_BATCH_S_MIN = 4, SUM_BATCH_S_MAX = 32, SUM_BATCH_S_FORCE_MAX = 4096;
// slices from which on a longer slice is the faster one (measured, profiles/sum_batch_ab.txt)
constexpr uint32_t SUM_BATCH_FILL_SLICES = 1u << 13;
inline bool sum_batch_s_valid(long v) { return v >= 1 && v <= (long)SUM_BATCH_S_FORCE_MAX && (v & (v - 1)) == 0; }

// The default S for `total` points in k segments on a machine of `lanes` resident lanes (G1) / lane pairs (G2): the largest
// power of two in [SUM_BATCH_S_MIN, SUM_BATCH_S_MAX] that still gives min(lanes, SUM_BATCH_FILL_SLICES) slices, counting
// total / S of them, else SUM_BATCH_S_MIN.  At S = 32 the sum passes are about 1.4 / S of the additions; a smaller S shortens
// the chain of dependent additions (about 10 us each) that a small call waits for.  The first candidate asked for `lanes`
// slices; on the measured grid that kept S = 4 up to 2^18 points, where S = 8 or 16 takes 19 - 27 % less time: 2^13 slices already
// hide the chain.  (k does not enter: every non-empty segment is a slice at any S, so the slices beyond total / S are the
// same for every candidate.)
inline uint32_t sum_batch_slice_default(uint64_t total, size_t k, uint32_t lanes) {
  (void)k;
  const uint64_t fill = lanes < SUM_BATCH_FILL_SLICES ? lanes : SUM_BATCH_FILL_SLICES;
  for (uint32_t S = SUM_BATCH_S_MAX; S > SUM_BATCH_S_MIN; S /= 2)
    if (total / S >= fill) return S;
  return SUM_BATCH_S_MIN;
}

// MLHIP_SUM_BATCH_SLICE if it names a valid S, else the default rule
inline uint32_t sum_batch_slice_len(uint64_t total, size_t k, uint32_t lanes) {
  if (const char* e = getenv("MLHIP_SUM_BATCH_SLICE")) {
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end != e && sum_batch_s_valid(v)) return (uint32_t)v;
  }
  return sum_batch_slice_default(total, k, lanes);
}

// The slices of k segments at slice length S and the sum passes over their partials; stride[q] = the c of slice q's segment.
// false: the slice or group indices do not fit 32 bits.  offsets must have been checked (0 first, nondecreasing).
inline bool sum_batch_layout(MsmBatchLayout& L, std::vector<uint32_t>& stride, const uint64_t* offsets, size_t k, uint32_t S,
                             int G = MSM_BATCH_GROUP) {
  if (!msm_batch_layout_by(L, offsets, k, G, [S](uint64_t) { return (uint64_t)S; })) return false;
  stride.resize(L.chunks.size());
  size_t q = 0;
  for (size_t s = 0; s < k; s++) {
    const uint64_t a = offsets[s], m = offsets[s + 1] - a;
    const uint64_t c = (m + S - 1) / S;  // < 2^32: the slices of all segments are
    for (uint64_t j = 0; j < c; j++, q++) {
      L.chunks[q] = {a + j, (uint32_t)point_sum_lane_count(j, c, m), (uint32_t)j};
      stride[q] = (uint32_t)c;
    }
  }
  return q == L.chunks.size();
}

// one past the last row of a slice: what point_sum_lane takes as its n (count >= 1)
MLHIP_HD uint64_t sum_batch_slice_end(const MsmBatchChunk& ch, uint32_t stride) {
  return ch.first + (uint64_t)(ch.count - 1) * stride + 1;
}

// the row of `points` that position i of the call reads, for the slice ch
struct SumLoadPoints {
  MLHIP_HD uint64_t row(uint64_t i, const MsmBatchChunk&) const { return i; }
};
struct SumLoadIndexed {
  const uint32_t* index;  // the call's base indices, one per position
  MLHIP_HD uint64_t row(uint64_t i, const MsmBatchChunk&) const { return index[i]; }
};
struct SumLoadSegment {
  MLHIP_HD uint64_t row(uint64_t i, const MsmBatchChunk& ch) const { return i - (ch.first - ch.base0); }  // i - a
};

// acc = the sum of slice ch; read(p, r) reads row r of the points
template <class F, class Ops, class Load, class Read>
MLHIP_HD void sum_batch_slice(XYZZ<F>& acc, const MsmBatchChunk& ch, uint32_t stride, const Load& load, Read read) {
  point_sum_lane<F, Ops>(acc, (size_t)ch.first, (size_t)stride, (size_t)sum_batch_slice_end(ch, stride),
                         [&](Affine<F>& p, size_t i) { read(p, load.row(i, ch)); });
}

#if defined(__HIPCC__)
// ---- kernels ---------------------------------------------------------------------------------------------------------
template <class C, class Load>
__global__ void __launch_bounds__(64) k_sum_batch_slice(const Affine<FpField<C>>* __restrict__ points, Load load,
                                                        const MsmBatchChunk* __restrict__ chunks,
                                                        const uint32_t* __restrict__ stride, uint32_t n_chunks,
                                                        XYZZ<FpField<C>>* __restrict__ partials) {
  typedef FpField<C> F;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const MsmBatchChunk ch = chunks[c];
  XYZZ<F> acc;
  sum_batch_slice<F, MsmBatchOps<F>>(acc, ch, stride[c], load, [&](Affine<F>& p, uint64_t r) { p = points[r]; });
  partials[c] = acc;
}

template <class C, class Load>
__global__ void __launch_bounds__(64) k_sum_batch_slice_lp(const Affine<Fp2Field<C>>* __restrict__ points, Load load,
                                                           const MsmBatchChunk* __restrict__ chunks,
                                                           const uint32_t* __restrict__ stride, uint32_t n_chunks,
                                                           XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair share the slice
  if (c >= n_chunks) return;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchChunk ch = chunks[c];
  XYZZ<FL> acc;
  sum_batch_slice<FL, MsmBatchOpsLp<C>>(acc, ch, stride[c], load,
                                        [&](Affine<FL>& p, uint64_t r) { lp_load_affine<C>(p, points, r, hi); });
  lp_store_xyzz<C>(partials, c, acc, hi);
}

template <class C, class F, class Load>
void sum_batch_launch(const void* d_points, Load load, const MsmBatchChunk* d_chunks, const uint32_t* d_stride, uint32_t n_chunks,
                      void* d_partials, hipStream_t st) {
  if constexpr (std::is_same<F, FpField<C>>::value)
    k_sum_batch_slice<C, Load><<<dim3((n_chunks + 63) / 64), dim3(64), 0, st>>>(
        (const Affine<FpField<C>>*)d_points, load, d_chunks, d_stride, n_chunks, (XYZZ<FpField<C>>*)d_partials);
  else
    k_sum_batch_slice_lp<C, Load><<<dim3((unsigned)((2 * (size_t)n_chunks + 63) / 64)), dim3(64), 0, st>>>(
        (const Affine<Fp2Field<C>>*)d_points, load, d_chunks, d_stride, n_chunks, (XYZZ<Fp2Field<C>>*)d_partials);
}

// The flagged batch calls behind their checks (api_msm.hip, api_bases.hip): k >= 1 checked offsets; bases = false: position i
// reads d_points[i]; bases = true: d_points are a handle's points, read through base_index (host, within the handle) or, when
// it is null, by the position in the segment.  Neither scalars nor the handle's batch tables are touched.
template <class C, class F>
int sum_batch_device(const void* d_points, bool bases, const uint32_t* base_index, const uint64_t* offsets, size_t k, void* d_out,
                     hipStream_t st) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  const uint32_t S = sum_batch_slice_len(offsets[k], k, kG1 ? POINT_SUM_MAX_LANES_G1 : POINT_SUM_MAX_LANES_G2);
  MsmBatchLayout L;
  std::vector<uint32_t> extra;  // [the stride of every slice | the index list]
  if (!sum_batch_layout(L, extra, offsets, k, S)) return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: more than 2^32 - 1 chunks");
  const size_t n_slices = extra.size();
  if (bases && base_index) extra.insert(extra.end(), base_index, base_index + offsets[k]);
  return msm_batch_run<C, F>(L, extra.data(), extra.size() * sizeof(uint32_t), d_out, st,
                             [&](const MsmBatchChunk* d_chunks, uint32_t n_chunks, const void* d_extra, void* part, void*) {
    const uint32_t* d_stride = (const uint32_t*)d_extra;
    if (!bases)
      sum_batch_launch<C, F>(d_points, SumLoadPoints{}, d_chunks, d_stride, n_chunks, part, st);
    else if (base_index)
      sum_batch_launch<C, F>(d_points, SumLoadIndexed{d_stride + n_slices}, d_chunks, d_stride, n_chunks, part, st);
    else
      sum_batch_launch<C, F>(d_points, SumLoadSegment{}, d_chunks, d_stride, n_chunks, part, st);
  });
}
#endif  // __HIPCC__

}  // namespace mlhip
