// point_sum.h -- the device route of mlhip_g1_sum / mlhip_g2_sum: out = sum of n affine points, no scalars.
// Part of msm_kernels.h (after msm_batch.h).  The plan and the per-lane body above the kernels are plain C++ /
// __host__ __device__, so tests/hostmath_sum replays them on the CPU.  Layout, cost model and measurements: DESIGN.md
// section 13.
//
//   pass 0     lane t (G1) or lane pair t (G2, msm_g2.h) of L reads the points t, t + L, t + 2 L, ... -- one step of a wave
//              reads neighbouring rows -- and adds them into one XYZZ accumulator with the complete mixed addition
//              (xyzz_madd: first point, infinity, doubling and P + (-P) are branches of it, nothing assumes generic
//              position).  L partials are written in XYZZ.
//   sum passes the segment-sum passes of msm_batch.h over ONE segment of L partials (msm_batch_layout with k = 1, P = 1):
//              groups of at most MSM_BATCH_GROUP, the last pass converts to affine with one inversion.
//   L          point_sum_plan: the L of 32, 64, 128, ... up to the lanes the machine runs at once that makes the longest
//              chain of dependent additions -- ceil(n / L) in pass 0 plus the chains of the sum passes -- shortest.
#pragma once
#include <cstddef>
#include <cstdint>

#include "msm_batch.h"

namespace mlhip {

// lanes (G1) / lane pairs (G2) one launch keeps resident: 256 compute units x 4 SIMDs x one wave of 64 lanes.  More lanes
// than that run one after the other, so a larger L buys nothing.
constexpr uint32_t POINT_SUM_MAX_LANES_G1 = 65536, POINT_SUM_MAX_LANES_G2 = 32768;
constexpr uint32_t POINT_SUM_MIN_LANES = 32;

struct PointSumPlan {
  uint32_t L;      // lanes (lane pairs) of pass 0 = partials handed to the sum passes
  uint64_t S;      // slice length: the most points one lane adds, ceil(n / L)
  uint64_t chain;  // dependent additions from the first point to the result: S + the sum passes' group lengths
};

// dependent additions of the sum passes over m partials of one segment (msm_batch_layout's passes, k = 1)
inline uint64_t point_sum_pass_chain(uint64_t m, int G = MSM_BATCH_GROUP) {
  uint64_t chain = 0;
  while (m > (uint64_t)G) {
    chain += (uint64_t)G;
    m = (m + (uint64_t)G - 1) / (uint64_t)G;
  }
  return chain + m;
}

// n >= 1.  Ties go to the smaller L (fewer passes, less scratch).
inline PointSumPlan point_sum_plan(size_t n, uint32_t max_lanes, int G = MSM_BATCH_GROUP) {
  PointSumPlan best = {0, 0, 0};
  for (uint32_t L = POINT_SUM_MIN_LANES; L <= max_lanes; L *= 2) {
    const uint64_t S = ((uint64_t)n + L - 1) / L;
    const uint64_t chain = S + point_sum_pass_chain(L, G);
    if (!best.L || chain < best.chain) best = {L, S, chain};
    if (S <= 1) break;  // every lane has at most one point: more lanes only lengthen the sum passes
  }
  return best;
}

// points lane t of L adds: t, t + L, ... below n
MLHIP_HD uint64_t point_sum_lane_count(uint64_t t, uint64_t L, uint64_t n) { return t < n ? (n - t + L - 1) / L : 0; }

// acc = sum of the points t, t + L, t + 2 L, ... < n; load(p, i) reads point i.  The next point is loaded before the
// current addition (as in msm_accumulate_range), so the read overlaps the arithmetic.
template <class F, class Ops, class Load>
MLHIP_HD void point_sum_lane(XYZZ<F>& acc, size_t t, size_t L, size_t n, Load load) {
  xyzz_set_inf<F>(acc);
  if (t >= n) return;
  Affine<F> p;
  load(p, t);
#pragma unroll 1
  for (size_t i = t; i < n; i += L) {
    Affine<F> pn = p;
    if (n - i > L) load(pn, i + L);  // i + L < n, written so that it cannot wrap
    Ops::madd(acc, p);
    p = pn;
  }
}

#if defined(__HIPCC__)
// ---- kernels ---------------------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(64) k_point_sum(const Affine<FpField<C>>* __restrict__ points, size_t n, uint32_t L,
                                                  XYZZ<FpField<C>>* __restrict__ partials) {
  typedef FpField<C> F;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L) return;
  XYZZ<F> acc;
  point_sum_lane<F, MsmBatchOps<F>>(acc, t, L, n, [&](Affine<F>& p, size_t i) { p = points[i]; });
  partials[t] = acc;
}

template <class C>
__global__ void __launch_bounds__(64) k_point_sum_lp(const Affine<Fp2Field<C>>* __restrict__ points, size_t n, uint32_t L,
                                                     XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair share the slice
  if (t >= L) return;
  const int hi = (int)(threadIdx.x & 1u);
  XYZZ<FL> acc;
  point_sum_lane<FL, MsmBatchOpsLp<C>>(acc, t, L, n, [&](Affine<FL>& p, size_t i) { lp_load_affine<C>(p, points, i, hi); });
  lp_store_xyzz<C>(partials, t, acc, hi);
}

// d_out = the affine sum of the n >= 1 device points at d_points, queued on st
template <class C, class F>
int point_sum_device(const void* d_points, size_t n, void* d_out, hipStream_t st) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  const PointSumPlan plan = point_sum_plan(n, kG1 ? POINT_SUM_MAX_LANES_G1 : POINT_SUM_MAX_LANES_G2);
  const uint64_t offsets[2] = {0, plan.L};  // one segment of L one-partial "chunks": the sum passes over the L partials
  MsmBatchLayout lay;
  if (!msm_batch_layout(lay, offsets, 1, 1)) return mlhip_rt::fail(MLHIP_EINVAL, "point sum: layout");
  return msm_batch_run<C, F>(lay, nullptr, 0, d_out, st, [&](const MsmBatchChunk*, uint32_t n_partials, const void*, void* part, void*) {
    if constexpr (kG1)
      k_point_sum<C><<<dim3((n_partials + 63) / 64), dim3(64), 0, st>>>((const Affine<FpField<C>>*)d_points, n, n_partials,
                                                                        (XYZZ<FpField<C>>*)part);
    else
      k_point_sum_lp<C><<<dim3((unsigned)((2 * (size_t)n_partials + 63) / 64)), dim3(64), 0, st>>>(
          (const Affine<Fp2Field<C>>*)d_points, n, n_partials, (XYZZ<Fp2Field<C>>*)part);
  });
}
#endif  // __HIPCC__

}  // namespace mlhip
