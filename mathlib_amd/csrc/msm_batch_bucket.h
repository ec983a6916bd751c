// msm_batch_bucket.h -- the bucket (Pippenger) route for the long segments of mlhip_msm_batch* (G1).  Part of msm_kernels.h
// (after msm_batch.h).  The layout, the plan and every per-lane body above the kernels are plain C++ / __host__ __device__, so
// tests/hostmath_bucket replays them on the CPU.  Cost model and measurements: DESIGN.md section 8.
//
//   rows       a segment of at least T pairs is cut into slices of at most S pairs, every other segment into Straus chunks of
//              at most P pairs as before.  Both are rows of the one MsmBatchChunk table, contiguous per segment, so the sum
//              passes of msm_batch.h run unchanged.  T > 8 >= P: a row with count > P is a slice and belongs to the kernels
//              below, any other row to k_msm_batch_chunk (which skips the slices).  The short last slice of a long segment may
//              therefore be a Straus chunk; both are exact for it.  The rows that are slices travel in msm_batch_run's extra
//              upload.
//   digits     one lane per pair of a slice: fr_canonical, then the W = ceil((FR_BITS + 1) / 7) balanced signed windows of
//              the large MSM (msm_win_layout, msm_window_digit), one byte per pair and window: 0 = skip, else
//              (magnitude << 1) | negative, magnitude 1 .. 64.  Window-major per slice, every window's row padded with zero
//              bytes to a multiple of 16.
//   buckets    one wave per (slice, window), lane b owns bucket b (magnitude b + 1) in registers.  Every lane walks its
//              window's row with a cursor of its own, 16 bytes per load, compares in registers, loads the point of its next
//              match; the lanes rejoin and each adds its point with the complete mixed addition (xyzz_madd: first point,
//              infinity, doubling and P + (-P) are branches of it), the sign from the digit byte.  The only data-dependent
//              address is a pair index inside the slice.
//   reduce     S_w = sum_b (b + 1) B_b inside the wave: twelve times "v += the value of lane + d, infinity beyond lane 63",
//              d = 1, 2, .., 32 twice.  The first six steps leave the suffix sums B_b + .. + B_63 in the lanes, the second six
//              their sum in lane 0, which writes the window sum in XYZZ.
//   combine    one lane per slice: Horner from the top window down (msm_win_bits doublings, then one addition) into the
//              slice's row of the partials.
//   scratch    W rows of pad16(the longest slice) bytes + W XYZZ per slice, behind the partials in msm_batch.h's per-device
//              buffer.  A call that would need more than MSM_BATCH_BUCKET_SCRATCH_MAX for it takes the Straus
//              chunks for every segment (the same bytes).
// G2 and the table-free path of mlhip_bases_msm_batch* keep the Straus chunks.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "msm_batch.h"

namespace mlhip {

constexpr int MSM_BATCH_BUCKET_C = 7;         // digit width: 64 buckets, one per lane of a wave
constexpr uint32_t MSM_BATCH_BUCKET_LANES = 64;
constexpr uint32_t MSM_BATCH_BUCKET_MIN_FLOOR = 9;  // T > 8 >= P keeps "count > P" a sound test for a slice
// The defaults come from profiles/msm_batch_bucket_ab.txt.  MIN: the smallest measured segment length
// from which the route is more than 4 % ahead of the Straus chunks at every larger one, on all three curves, from 2^18 pairs
// per call on.  SLICE_MAX: the best slice of the sweep where the batch is large (2^20 pairs); longer slices lose waves
// faster than they fill buckets.
constexpr uint32_t MSM_BATCH_BUCKET_MIN_DEFAULT = 512;
constexpr uint32_t MSM_BATCH_BUCKET_SLICE_MIN = 256, MSM_BATCH_BUCKET_SLICE_MAX = 4096;
// (slice, window) waves the plan wants before it lengthens the slices: two rounds of the 256 compute units x 4 SIMDs x 2
// waves the accumulation kernel keeps resident (at 2^18 pairs slices of 2048, 4736 waves, beat slices of 4096 by 7-10 %)
constexpr uint64_t MSM_BATCH_BUCKET_WAVES = 4096;
constexpr size_t MSM_BATCH_BUCKET_SCRATCH_MAX = (size_t)1 << 30;

struct MsmBatchBucketPlan {
  uint32_t T;  // segments of at least T pairs are cut into slices; 0 = none (every segment keeps its Straus chunks)
  uint32_t S;  // pairs per slice, > P
};

// t_req: MLHIP_MSM_BATCH_BUCKET_MIN (< 0: the default; 0: never; 1 .. 8 mean 9), s_req: MLHIP_MSM_BATCH_BUCKET_SLICE (<= 0:
// the plan's own).  The plan's S is the largest power of two between SLICE_MIN and SLICE_MAX that still gives
// MSM_BATCH_BUCKET_WAVES (slice, window) waves -- long slices mean fuller buckets, so fewer lanes of a wave wait for the
// longest one and the 12 additions of the reduction are shared by more pairs -- and SLICE_MIN where the batch is too small
// for that.  A fixed S is raised to P + 1: a slice is a row with count > P.
inline MsmBatchBucketPlan msm_batch_bucket_plan(const uint64_t* offsets, size_t k, int P, int W, long t_req, long s_req) {
  MsmBatchBucketPlan plan = {MSM_BATCH_BUCKET_MIN_DEFAULT, MSM_BATCH_BUCKET_SLICE_MIN};
  if (t_req >= 0) plan.T = t_req > 0xffffffffL ? 0xffffffffu : (uint32_t)t_req;
  if (plan.T && plan.T < MSM_BATCH_BUCKET_MIN_FLOOR) plan.T = MSM_BATCH_BUCKET_MIN_FLOOR;
  if (!plan.T) return plan;
  if (s_req > 0) {
    plan.S = s_req > 0x40000000L ? 0x40000000u : (uint32_t)s_req;
    if (plan.S <= (uint32_t)P) plan.S = (uint32_t)P + 1;
    return plan;
  }
  for (uint32_t S = MSM_BATCH_BUCKET_SLICE_MAX; S > MSM_BATCH_BUCKET_SLICE_MIN; S /= 2) {
    uint64_t slices = 0;
    for (size_t s = 0; s < k; s++) {
      const uint64_t m = offsets[s + 1] - offsets[s];
      if (m >= plan.T) slices += (m + S - 1) / S;
    }
    if (slices * (uint64_t)W >= MSM_BATCH_BUCKET_WAVES) {
      plan.S = S;
      break;
    }
  }
  return plan;
}

// The rows of a call under a plan: msm_batch_layout with the plan's slice length for the long segments.  slices = the rows
// the bucket kernels write (count > P), in order.  plan.T = 0 (or no long segment) gives msm_batch_layout's tables.
inline bool msm_batch_bucket_layout(MsmBatchLayout& L, std::vector<uint32_t>& slices, const uint64_t* offsets, size_t k, int P,
                                    const MsmBatchBucketPlan& plan, int G = MSM_BATCH_GROUP) {
  slices.clear();
  if (!msm_batch_layout_by(L, offsets, k, G, [&](uint64_t m) { return plan.T && m >= plan.T ? (uint64_t)plan.S : (uint64_t)P; }))
    return false;
  for (size_t c = 0; c < L.chunks.size(); c++)
    if (L.chunks[c].count > (uint32_t)P) slices.push_back((uint32_t)c);
  return true;
}

// ---- scratch -----------------------------------------------------------------------------------------------------------
MLHIP_HD uint32_t msm_bucket_pad16(uint32_t n) { return (n + 15u) & ~15u; }
// bytes of one slice's digit table: W rows of pad16(n) bytes, n = the longest slice of the call
MLHIP_HD size_t msm_bucket_digit_stride(uint32_t n, int W) { return (size_t)W * msm_bucket_pad16(n); }

// ---- digits ------------------------------------------------------------------------------------------------------------
// lane j of a slice of count pairs, j < pad16(count): the W digit bytes of pair j into rows[w * row_bytes + j]; the lanes
// past the slice's end write the zero bytes the 16-byte scan reads.  scalars = the slice's first scalar.
template <class C>
MLHIP_HD void msm_bucket_digits(uint8_t* rows, uint32_t row_bytes, uint32_t j, uint32_t count, const uint32_t* scalars, bool mont) {
  const WinLayout l = msm_win_layout(C::FR_BITS, MSM_BATCH_BUCKET_C);
  uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (j < count) fr_canonical<C>(s, scalars + 8 * (size_t)j, mont);  // past the end: s = 0, every digit 0
  uint32_t carry = 0, neg = 0;
  for (int w = 0; w < l.W; w++) {
    const uint32_t mag = msm_window_digit(s, msm_win_off(l.base, l.rem, w), msm_win_bits(l.base, l.rem, w), carry, neg);
    rows[(size_t)w * row_bytes + j] = (uint8_t)(mag ? ((mag << 1) | neg) : 0u);
  }
}

// ---- buckets -----------------------------------------------------------------------------------------------------------
struct alignas(16) MsmBucketBytes16 {
  uint32_t w[4];
};

// The first pair at or after cur whose byte in row has the magnitude mag (1 .. 64); n16 (= pad16 of the slice's count, the
// row's zero padding included) when there is none.  neg = the byte's sign bit.  row is 16-byte aligned; 16 bytes per load.
MLHIP_HD uint32_t msm_bucket_scan(const uint8_t* row, uint32_t cur, uint32_t n16, uint32_t mag, uint32_t& neg) {
  const uint32_t want = mag << 1;
  while (cur < n16) {
    const uint32_t base = cur & ~15u;
    const MsmBucketBytes16 g = *reinterpret_cast<const MsmBucketBytes16*>(row + base);
    uint32_t hit = 0, sign = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t b = (g.w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      hit |= (uint32_t)((b & 0xfeu) == want) << i;
      sign |= (b & 1u) << i;
    }
    hit &= 0xffffu << (cur & 15u);  // the bytes before the cursor have been taken
    if (hit) {
      const uint32_t i = (uint32_t)__builtin_ctz(hit);
      neg = (sign >> i) & 1u;
      return base + i;
    }
    cur = base + 16u;
  }
  return n16;
}

// acc = the sum of the slice's points whose digit in this window has magnitude lane + 1, each negated where its digit is
// negative; load(p, j) reads pair j of the slice.  On the device the lanes of a wave leave the scan together and add side by
// side; the host runs one lane after the other.
template <class F, class Load>
MLHIP_HD void msm_bucket_lane(XYZZ<F>& acc, const uint8_t* row, uint32_t n16, uint32_t lane, Load load) {
  xyzz_set_inf<F>(acc);
  uint32_t cur = 0;
#pragma unroll 1
  for (;;) {
    uint32_t neg = 0;
    const uint32_t j = msm_bucket_scan(row, cur, n16, lane + 1u, neg);
    if (j >= n16) break;
    Affine<F> p;
    load(p, j);
    xyzz_madd<F>(acc, p, neg != 0);
    cur = j + 1u;
  }
}

// ---- reduction ---------------------------------------------------------------------------------------------------------
constexpr int MSM_BATCH_BUCKET_REDUCE_STEPS = 12;
// One step of the 64-lane reduction, run by every lane: v += the v of lane + d (infinity beyond lane 63), d = 2^(step mod 6).
// neighbour(q, v, d) fetches that value as it was before the step.  After steps 0 .. 5 lane b holds B_b + .. + B_63, after
// steps 6 .. 11 lane 0 holds their sum = sum_b (b + 1) B_b.
template <class F, class Ops, class Neighbour>
MLHIP_HD void msm_bucket_reduce_step(XYZZ<F>& v, int step, Neighbour neighbour) {
  XYZZ<F> q;
  neighbour(q, v, 1u << (step % 6));
  Ops::add(v, q);
}

// ---- window combination ------------------------------------------------------------------------------------------------
// acc = sum_w 2^off(w) S_w, load(q, w) reading the window sum S_w: Horner from the top window down
template <class F, class Ops, class Load>
MLHIP_HD void msm_bucket_combine(XYZZ<F>& acc, int fr_bits, Load load) {
  const WinLayout l = msm_win_layout(fr_bits, MSM_BATCH_BUCKET_C);
  xyzz_set_inf<F>(acc);
#pragma unroll 1
  for (int w = l.W - 1; w >= 0; w--) {
    const int bits = msm_win_bits(l.base, l.rem, w);
#pragma unroll 1
    for (int d = 0; d < bits; d++) {
      XYZZ<F> t;
      Ops::dbl(t, acc);
      acc = t;
    }
    XYZZ<F> q;
    load(q, w);
    Ops::add(acc, q);
  }
}

#if defined(__HIPCC__)
// ---- kernels ---------------------------------------------------------------------------------------------------------
// blocks_per_slice blocks of 64 lanes per slice (pad16(S) lanes rounded up): lane j of slice i takes pair j
template <class C>
__global__ void __launch_bounds__(64) k_msm_bucket_digits(const uint32_t* __restrict__ scalars, int mont,
                                                          const MsmBatchChunk* __restrict__ chunks,
                                                          const uint32_t* __restrict__ slice_rows, uint32_t n_slices,
                                                          uint32_t blocks_per_slice, uint32_t row_bytes, int W,
                                                          uint8_t* __restrict__ digits) {
  const uint32_t i = blockIdx.x / blocks_per_slice;
  const uint32_t j = (blockIdx.x % blocks_per_slice) * 64u + threadIdx.x;
  if (i >= n_slices) return;
  const MsmBatchChunk ch = chunks[slice_rows[i]];
  if (j >= msm_bucket_pad16(ch.count)) return;  // <= row_bytes = pad16(the longest slice)
  msm_bucket_digits<C>(digits + (size_t)i * W * row_bytes, row_bytes, j, ch.count, scalars + 8 * ch.first, mont != 0);
}

template <class F>
struct MsmBucketOps {
  __device__ __noinline__ static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  __device__ static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
};

// one wave per (slice, window): block = slice * W + window
template <class C>
__global__ void __launch_bounds__(64) k_msm_bucket_accumulate(const Affine<FpField<C>>* __restrict__ points,
                                                              const MsmBatchChunk* __restrict__ chunks,
                                                              const uint32_t* __restrict__ slice_rows, uint32_t row_bytes, int W,
                                                              const uint8_t* __restrict__ digits,
                                                              XYZZ<FpField<C>>* __restrict__ window_sums) {
  typedef FpField<C> F;
  constexpr int WORDS = (int)(sizeof(XYZZ<F>) / sizeof(uint32_t));
  const uint32_t i = blockIdx.x / (uint32_t)W, w = blockIdx.x % (uint32_t)W;
  const uint32_t lane = threadIdx.x;
  const MsmBatchChunk ch = chunks[slice_rows[i]];
  const Affine<F>* pts = points + ch.first;
  const uint8_t* row = digits + ((size_t)i * W + w) * row_bytes;
  XYZZ<F> v;
  msm_bucket_lane<F>(v, row, msm_bucket_pad16(ch.count), lane, [&](Affine<F>& p, uint32_t j) { p = pts[j]; });
  XYZZ<F> inf;
  xyzz_set_inf<F>(inf);
#pragma unroll 1
  for (int step = 0; step < MSM_BATCH_BUCKET_REDUCE_STEPS; step++)
    msm_bucket_reduce_step<F, MsmBucketOps<F>>(v, step, [&](XYZZ<F>& q, const XYZZ<F>& mine, uint32_t d) {
      const uint32_t* a = reinterpret_cast<const uint32_t*>(&mine);
      const uint32_t* z = reinterpret_cast<const uint32_t*>(&inf);
      uint32_t* b = reinterpret_cast<uint32_t*>(&q);
      const bool beyond = lane + d >= MSM_BATCH_BUCKET_LANES;
#pragma unroll
      for (int t = 0; t < WORDS; t++) {
        const uint32_t x = (uint32_t)__shfl_down((int)a[t], d, 64);
        b[t] = beyond ? z[t] : x;
      }
    });
  if (lane == 0) window_sums[(size_t)i * W + w] = v;
}

// one lane per slice
template <class C>
__global__ void __launch_bounds__(64) k_msm_bucket_combine(const XYZZ<FpField<C>>* __restrict__ window_sums,
                                                           const uint32_t* __restrict__ slice_rows, uint32_t n_slices, int W,
                                                           XYZZ<FpField<C>>* __restrict__ partials) {
  typedef FpField<C> F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slices) return;
  const XYZZ<F>* ws = window_sums + (size_t)i * W;
  XYZZ<F> acc;
  msm_bucket_combine<F, MsmBatchOpsG1<F>>(acc, C::FR_BITS, [&](XYZZ<F>& q, int w) { q = ws[w]; });
  partials[slice_rows[i]] = acc;
}

inline long msm_batch_env_long(const char* name) {
  const char* e = getenv(name);
  if (!e || !*e) return -1;
  const long v = atol(e);
  return v < 0 ? -1 : v;
}

// mlhip_msm_batch_device behind the ABI: G1 segments of at least T pairs through the bucket kernels, everything else (G2, a
// call without a long segment, a call whose scratch would pass the bound) as msm_batch_device has it.
template <class C, class F>
int msm_batch_route_device(const void* d_points, const void* d_scalars, int mont, const uint64_t* offsets, size_t k, void* d_out,
                           hipStream_t st) {
  if constexpr (!std::is_same<F, FpField<C>>::value) {
    return msm_batch_device<C, F>(d_points, d_scalars, mont, offsets, k, d_out, st);
  } else {
    const int P = msm_batch_chunk_len<C, F>();
    const int W = msm_win_layout(C::FR_BITS, MSM_BATCH_BUCKET_C).W;
    const MsmBatchBucketPlan plan = msm_batch_bucket_plan(offsets, k, P, W, msm_batch_env_long("MLHIP_MSM_BATCH_BUCKET_MIN"),
                                                          msm_batch_env_long("MLHIP_MSM_BATCH_BUCKET_SLICE"));
    if (!plan.T) return msm_batch_device<C, F>(d_points, d_scalars, mont, offsets, k, d_out, st);
    MsmBatchLayout L;
    std::vector<uint32_t> slices;
    if (!msm_batch_bucket_layout(L, slices, offsets, k, P, plan))
      return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: more than 2^32 - 1 chunks");
    if (slices.empty()) return msm_batch_device<C, F>(d_points, d_scalars, mont, offsets, k, d_out, st);
    const uint32_t n_slices = (uint32_t)slices.size();
    uint32_t longest = 0;  // <= S; shorter where every long segment is
    for (uint32_t c : slices) longest = L.chunks[c].count > longest ? L.chunks[c].count : longest;
    const uint32_t row_bytes = msm_bucket_pad16(longest);
    const uint32_t blocks_per_slice = (row_bytes + 63u) / 64u;
    const size_t digit_bytes = ((size_t)n_slices * msm_bucket_digit_stride(longest, W) + 255) & ~(size_t)255;
    const size_t scratch = digit_bytes + (size_t)n_slices * W * sizeof(XYZZ<F>);
    if (scratch > MSM_BATCH_BUCKET_SCRATCH_MAX || (uint64_t)n_slices * blocks_per_slice >= ((uint64_t)1 << 31) ||
        (uint64_t)n_slices * (uint64_t)W >= ((uint64_t)1 << 31))
      return msm_batch_device<C, F>(d_points, d_scalars, mont, offsets, k, d_out, st);
    return msm_batch_run<C, F>(
        L, slices.data(), slices.size() * sizeof(uint32_t), d_out, st,
        [&](const MsmBatchChunk* d_chunks, uint32_t n_chunks, const void* d_extra, void* part, void* d_scratch) {
          const uint32_t* d_rows = (const uint32_t*)d_extra;
          uint8_t* d_digits = (uint8_t*)d_scratch;
          XYZZ<F>* d_wsums = (XYZZ<F>*)((char*)d_scratch + digit_bytes);
          if (n_chunks > n_slices) msm_batch_launch_chunks_p<C, F>(P, d_points, d_scalars, mont, d_chunks, n_chunks, part, st);
          k_msm_bucket_digits<C><<<dim3(n_slices * blocks_per_slice), dim3(64), 0, st>>>(
              (const uint32_t*)d_scalars, mont, d_chunks, d_rows, n_slices, blocks_per_slice, row_bytes, W, d_digits);
          k_msm_bucket_accumulate<C><<<dim3(n_slices * (uint32_t)W), dim3(64), 0, st>>>(
              (const Affine<F>*)d_points, d_chunks, d_rows, row_bytes, W, d_digits, d_wsums);
          k_msm_bucket_combine<C><<<dim3((n_slices + 63) / 64), dim3(64), 0, st>>>(d_wsums, d_rows, n_slices, W, (XYZZ<F>*)part);
        },
        scratch);
  }
}
#endif  // __HIPCC__

}  // namespace mlhip
