// tests/hostmath_sum_batch -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the segmented point
// sums' slice layout, choice of S and slice body (mathlib_amd/csrc/msm_sum_batch.h), replayed on the CPU slice by slice in
// the order the kernels run them: sum_batch_layout cuts the segments, sum_batch_slice per slice through one of the three
// loads, then the sum passes of msm_batch.h over the slice partials (msm_batch_sum per group; xyzz_to_affine in the last
// pass).  G2 runs the same bodies over one-lane Fp2 (the kernels use lane pairs).  Driven by tests/test_sum_batch_host.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_sum_batch.h"

using namespace mlhip;

static uint32_t max_lanes(int group) { return group == 1 ? POINT_SUM_MAX_LANES_G1 : POINT_SUM_MAX_LANES_G2; }

template <class F, class Load>
static void pass0(std::vector<XYZZ<F>>& part, const MsmBatchLayout& L, const std::vector<uint32_t>& stride, const Affine<F>* pts,
                  const Load& load) {
  for (size_t q = 0; q < L.chunks.size(); q++)
    sum_batch_slice<F, MsmBatchOps<F>>(part[q], L.chunks[q], stride[q], load, [&](Affine<F>& p, uint64_t r) { p = pts[r]; });
}

template <class F>
static int sums(const void* points, int mode, const uint32_t* index, const uint64_t* offsets, size_t k, uint32_t S, uint32_t lanes,
                void* out, uint64_t* stats) {
  if (k == 0) return -1;
  if (!S) S = sum_batch_slice_default(offsets[k], k, lanes);
  MsmBatchLayout L;
  std::vector<uint32_t> stride;
  if (!sum_batch_layout(L, stride, offsets, k, S)) return -2;
  const Affine<F>* pts = (const Affine<F>*)points;
  std::vector<XYZZ<F>> cur(L.chunks.size()), next;
  if (mode == 0)
    pass0<F>(cur, L, stride, pts, SumLoadPoints{});
  else if (mode == 1)
    pass0<F>(cur, L, stride, pts, SumLoadIndexed{index});
  else
    pass0<F>(cur, L, stride, pts, SumLoadSegment{});
  const size_t passes = L.pass_begin.size() - 1;
  for (size_t q = 0; q < passes; q++) {
    const size_t g0 = L.pass_begin[q], g1 = L.pass_begin[q + 1];
    if (q + 1 == passes && g1 - g0 != k) return -3;
    next.assign(g1 - g0, XYZZ<F>());
    for (size_t g = g0; g < g1; g++) {
      const MsmBatchGroup gr = L.groups[g];
      if ((size_t)gr.begin + gr.count > cur.size()) return -4;
      msm_batch_sum<F, MsmBatchOps<F>>(next[g - g0], gr.count, [&](XYZZ<F>& p, uint32_t i) { p = cur[gr.begin + i]; });
    }
    cur.swap(next);
  }
  for (size_t s = 0; s < k; s++) xyzz_to_affine<F>(((Affine<F>*)out)[s], cur[s]);
  if (stats) {
    stats[0] = S;
    stats[1] = L.chunks.size();
    stats[2] = passes;
  }
  return 0;
}

template <class C>
static int sums_group(int group, const void* points, int mode, const uint32_t* index, const uint64_t* offsets, size_t k, uint32_t S,
                      void* out, uint64_t* stats) {
  if (group == 1) return sums<FpField<C>>(points, mode, index, offsets, k, S, max_lanes(1), out, stats);
  return sums<Fp2Field<C>>(points, mode, index, offsets, k, S, max_lanes(2), out, stats);
}

extern "C" {
// out[s] = the affine sum of segment s, s < k.  mode 0: position i reads points[i]; 1: points[index[i]]; 2: points[i - a]
// (a = the segment's first position).  S = 0: the default rule.  stats = {S, slices, sum passes} (may be null)
int hsb_sum_batch(int curve, int group, const void* points, int mode, const uint32_t* index, const uint64_t* offsets, size_t k,
                  uint32_t S, void* out, uint64_t* stats) {
  switch (curve) {
    case 0: return sums_group<Bn254>(group, points, mode, index, offsets, k, S, out, stats);
    case 1: return sums_group<Bls381>(group, points, mode, index, offsets, k, S, out, stats);
    case 2: return sums_group<Bls377>(group, points, mode, index, offsets, k, S, out, stats);
    default: return -6;
  }
}

// The slice tables of k segments at slice length S, checked directly.  0: every position of every segment is read by
// exactly one slice, and by one of its own segment; a slice's count is the number of positions it reads, at least 1 and at
// most S; base0 is the slice's number in its segment; sum_batch_slice_end is one past its last position; the three loads
// give i, index[i] and i - a; the slices of a segment are contiguous and in segment order (what the sum passes assume); and
// no slice or group is longer than max(S, G).  stats = {slices, longest slice, longest group, sum passes}
int hsb_layout_check(const uint64_t* offsets, size_t k, uint32_t S, uint64_t* stats) {
  MsmBatchLayout L;
  std::vector<uint32_t> stride;
  if (!sum_batch_layout(L, stride, offsets, k, S)) return -1;
  if (stride.size() != L.chunks.size()) return -2;
  const uint64_t total = offsets[k];
  std::vector<uint8_t> seen(total, 0);
  std::vector<uint32_t> index(total);
  for (uint64_t i = 0; i < total; i++) index[i] = (uint32_t)(i * 2654435761u);
  size_t q = 0;
  uint64_t longest = 0;
  for (size_t s = 0; s < k; s++) {
    const uint64_t a = offsets[s], b = offsets[s + 1], m = b - a, c = (m + S - 1) / S;
    for (uint64_t j = 0; j < c; j++, q++) {
      if (q >= L.chunks.size()) return -3;
      const MsmBatchChunk ch = L.chunks[q];
      if (stride[q] != c || ch.first != a + j || ch.base0 != j) return -4;
      uint64_t count = 0, last = 0;
      for (uint64_t i = ch.first; i < b; i += stride[q]) {
        if (seen[i]) return -5;
        seen[i] = 1;
        count++;
        last = i;
        if (SumLoadPoints{}.row(i, ch) != i || SumLoadIndexed{index.data()}.row(i, ch) != index[i] ||
            SumLoadSegment{}.row(i, ch) != i - a)
          return -6;
      }
      if (count != ch.count || count < 1 || count > S) return -7;
      if (sum_batch_slice_end(ch, stride[q]) != last + 1 || last >= b) return -8;
      longest = count > longest ? count : longest;
    }
  }
  if (q != L.chunks.size()) return -9;
  for (uint64_t i = 0; i < total; i++)
    if (!seen[i]) return -10;
  // pass 0's groups tile the slices in order, every group inside one segment
  uint32_t most = 0;
  for (size_t g = 0; g < L.groups.size(); g++) most = L.groups[g].count > most ? L.groups[g].count : most;
  if (most > (uint32_t)MSM_BATCH_GROUP) return -11;
  {
    size_t g = L.pass_begin[0], at = 0;
    const bool last = L.pass_begin.size() == 2;
    for (size_t s = 0; s < k; s++) {
      const uint64_t c = (offsets[s + 1] - offsets[s] + S - 1) / S;
      uint64_t left = c;
      if (last) {
        if (L.groups[g].begin != at || L.groups[g].count != c) return -12;
        g++;
      } else {
        while (left) {
          if (g >= L.pass_begin[1] || L.groups[g].begin != at + (c - left) || L.groups[g].count > left) return -13;
          left -= L.groups[g].count;
          g++;
        }
      }
      at += c;
    }
    if (g != L.pass_begin[1]) return -14;
  }
  if (L.pass_begin.back() - L.pass_begin[L.pass_begin.size() - 2] != k) return -15;
  stats[0] = L.chunks.size();
  stats[1] = longest;
  stats[2] = most;
  stats[3] = L.pass_begin.size() - 1;
  return 0;
}

// the default S of a call of `total` points in k segments for the group
uint32_t hsb_slice_default(uint64_t total, size_t k, int group) { return sum_batch_slice_default(total, k, max_lanes(group)); }
// is v an S that MLHIP_SUM_BATCH_SLICE accepts
int hsb_slice_valid(long v) { return sum_batch_s_valid(v) ? 1 : 0; }
}
