// tests/hostmath_sum -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the plain point sum's
// plan and per-lane body (mathlib_amd/csrc/point_sum.h), replayed on the CPU lane by lane in the order the kernels run
// them: point_sum_plan picks L, point_sum_lane per lane, then the sum passes of msm_batch.h over the L partials
// (msm_batch_layout with k = 1, P = 1; msm_batch_sum per group; xyzz_to_affine in the last pass).  G2 runs the same bodies
// over one-lane Fp2 (the kernels use lane pairs).  Driven by tests/test_point_sum_host.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/point_sum.h"

using namespace mlhip;

static uint32_t max_lanes(int group) { return group == 1 ? POINT_SUM_MAX_LANES_G1 : POINT_SUM_MAX_LANES_G2; }

template <class F>
static int sum(const void* points, size_t n, uint32_t max_l, uint32_t force_l, void* out, uint64_t* stats) {
  if (n == 0) return -1;
  PointSumPlan plan = point_sum_plan(n, max_l);
  if (force_l) plan = {force_l, (n + force_l - 1) / force_l, 0};
  const Affine<F>* pts = (const Affine<F>*)points;
  std::vector<XYZZ<F>> cur(plan.L), next;
  for (uint32_t t = 0; t < plan.L; t++)
    point_sum_lane<F, MsmBatchOps<F>>(cur[t], t, plan.L, n, [&](Affine<F>& p, size_t i) { p = pts[i]; });
  const uint64_t offsets[2] = {0, plan.L};
  MsmBatchLayout lay;
  if (!msm_batch_layout(lay, offsets, 1, 1)) return -2;
  if (lay.chunks.size() != plan.L) return -3;
  const size_t passes = lay.pass_begin.size() - 1;
  for (size_t q = 0; q < passes; q++) {
    const size_t g0 = lay.pass_begin[q], g1 = lay.pass_begin[q + 1];
    if (q + 1 == passes && g1 - g0 != 1) return -4;
    next.assign(g1 - g0, XYZZ<F>());
    for (size_t g = g0; g < g1; g++) {
      const MsmBatchGroup gr = lay.groups[g];
      if ((size_t)gr.begin + gr.count > cur.size()) return -5;
      msm_batch_sum<F, MsmBatchOps<F>>(next[g - g0], gr.count, [&](XYZZ<F>& p, uint32_t i) { p = cur[gr.begin + i]; });
    }
    cur.swap(next);
  }
  xyzz_to_affine<F>(*(Affine<F>*)out, cur[0]);
  if (stats) {
    stats[0] = plan.L;
    stats[1] = plan.S;
    stats[2] = passes;
  }
  return 0;
}

template <class C>
static int sum_group(int group, const void* points, size_t n, uint32_t force_l, void* out, uint64_t* stats) {
  if (group == 1) return sum<FpField<C>>(points, n, max_lanes(1), force_l, out, stats);
  return sum<Fp2Field<C>>(points, n, max_lanes(2), force_l, out, stats);
}

extern "C" {
// out = the affine sum of the n >= 1 points; force_l != 0 replaces the plan's L; stats = {L, S, sum passes} (may be null)
int hms_point_sum(int curve, int group, const void* points, size_t n, uint32_t force_l, void* out, uint64_t* stats) {
  switch (curve) {
    case 0: return sum_group<Bn254>(group, points, n, force_l, out, stats);
    case 1: return sum_group<Bls381>(group, points, n, force_l, out, stats);
    case 2: return sum_group<Bls377>(group, points, n, force_l, out, stats);
    default: return -6;
  }
}

// The plan of n points (force_l != 0: that L instead) and what its lanes read: plan = {L, S, chain}.  0: every index below n
// is read by exactly one lane, no lane reads more than S points, one reads exactly S, the counts are point_sum_lane_count's,
// and the chain is S + the group lengths of msm_batch_layout's passes over L partials.
int hms_plan_check(int group, size_t n, uint32_t force_l, uint64_t* plan_out) {
  if (n == 0) return -1;
  PointSumPlan plan = point_sum_plan(n, max_lanes(group));
  if (force_l) plan = {force_l, (n + force_l - 1) / force_l, ((uint64_t)n + force_l - 1) / force_l + point_sum_pass_chain(force_l)};
  plan_out[0] = plan.L;
  plan_out[1] = plan.S;
  plan_out[2] = plan.chain;
  if (plan.L < 1 || plan.L > max_lanes(group)) return -2;
  std::vector<uint8_t> seen(n, 0);
  uint64_t longest = 0;
  for (uint64_t t = 0; t < plan.L; t++) {
    uint64_t count = 0;
    for (uint64_t i = t; i < n; i += plan.L) {
      if (seen[i]) return -3;
      seen[i] = 1;
      count++;
    }
    if (count != point_sum_lane_count(t, plan.L, n)) return -4;
    longest = count > longest ? count : longest;
  }
  for (size_t i = 0; i < n; i++)
    if (!seen[i]) return -5;
  if (longest != plan.S) return -6;
  const uint64_t offsets[2] = {0, plan.L};
  MsmBatchLayout lay;
  if (!msm_batch_layout(lay, offsets, 1, 1)) return -7;
  uint64_t chain = plan.S;
  for (size_t q = 0; q + 1 < lay.pass_begin.size(); q++) {
    uint32_t most = 0;
    for (size_t g = lay.pass_begin[q]; g < lay.pass_begin[q + 1]; g++) most = lay.groups[g].count > most ? lay.groups[g].count : most;
    chain += most;
  }
  if (chain != plan.chain) return -8;
  return 0;
}
}
