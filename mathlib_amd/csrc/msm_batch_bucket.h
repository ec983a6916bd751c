// msm_batch_bucket.h -- the bucket (Pippenger) route for the long segments of mlhip_msm_batch* (G1 and G2) and of the table-free
// path of mlhip_bases_msm_batch* (msm_bases_batch.h).  Part of msm_kernels.h (after msm_batch.h).  The layout, the plan and every per-lane body above the kernels are plain C++ / __host__ __device__, so
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
//   G2         the same bodies over lane pairs (Fp2LField, one Fp2 component per lane, as the G2 chunk kernels): a wave is 32
//              pairs, so 6-bit signed windows (W = 43 on all three curves), 32 buckets, lane pair b owns bucket b; both lanes
//              of a pair run the identical scan, so every branch is pair-uniform.  Ten reduction steps (d = 1 .. 16 pairs
//              twice, __shfl_down by 2 d lanes: a lane receives its own component); one lane pair per slice for Horner.
//   bases      the table-free path of mlhip_bases_msm_batch* runs the same kernels with the point of pair j read through
//              the call's index list (MsmBucketIndexed); the index list travels in front of the slice rows.
//   defaults   per group (MsmBucketShape<G1>::tuning()): profiles/msm_batch_bucket_ab.txt, profiles/msm_batch_bucket_g2_ab.txt.
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

// What differs between the groups: the digit width (one bucket per lane of a wave for G1, per lane pair for G2), hence the
// steps of the in-wave reduction, and the compiled defaults of the plan.
struct MsmBatchBucketTuning {
  uint32_t min_default;           // MLHIP_MSM_BATCH_BUCKET_MIN unset: segments from this many pairs on (0 = never: opt-in)
  uint32_t slice_min, slice_max;  // the plan's own slice length lies between these
  uint64_t waves;                 // (slice, window) waves the plan wants before it lengthens the slices
};
constexpr int MSM_BATCH_BUCKET_C_G2 = 6;  // 32 buckets, one per lane pair of a wave
// G2 defaults: profiles/msm_batch_bucket_g2_ab.txt, by the rules of the G1 values above.  MIN: ahead by
// more than 4 % from 256 pairs per segment on, all three curves, at 2^16 and 2^18 pairs per call.  SLICE_MAX: at 2^18 pairs in
// 16 segments slices of 1024 and 2048 are level (1024 ahead by 0-6 % over two runs) and 4096 is 14-27 % behind: a wave of 32
// buckets is filled sooner than one of 64.  The accumulation kernel keeps the same 2 waves per SIMD resident, so the wave
// target stays.
constexpr uint32_t MSM_BATCH_BUCKET_MIN_DEFAULT_G2 = 256;
constexpr uint32_t MSM_BATCH_BUCKET_SLICE_MIN_G2 = 256, MSM_BATCH_BUCKET_SLICE_MAX_G2 = 1024;
constexpr uint64_t MSM_BATCH_BUCKET_WAVES_G2 = 4096;
template <bool G1>
struct MsmBucketShape {
  static constexpr int WIDTH = G1 ? MSM_BATCH_BUCKET_C : MSM_BATCH_BUCKET_C_G2;
  static constexpr int LOG = WIDTH - 1;           // log2 of the buckets
  static constexpr uint32_t BUCKETS = 1u << LOG;  // = the lanes (G1) or lane pairs (G2) of a wave
  static constexpr int STEPS = 2 * LOG;           // of the in-wave reduction
  static constexpr MsmBatchBucketTuning tuning() {
    return G1 ? MsmBatchBucketTuning{MSM_BATCH_BUCKET_MIN_DEFAULT, MSM_BATCH_BUCKET_SLICE_MIN, MSM_BATCH_BUCKET_SLICE_MAX,
                                     MSM_BATCH_BUCKET_WAVES}
              : MsmBatchBucketTuning{MSM_BATCH_BUCKET_MIN_DEFAULT_G2, MSM_BATCH_BUCKET_SLICE_MIN_G2,
                                     MSM_BATCH_BUCKET_SLICE_MAX_G2, MSM_BATCH_BUCKET_WAVES_G2};
  }
};

struct MsmBatchBucketPlan {
  uint32_t T;  // segments of at least T pairs are cut into slices; 0 = none (every segment keeps its Straus chunks)
  uint32_t S;  // pairs per slice, > P
};

// t_req: MLHIP_MSM_BATCH_BUCKET_MIN (< 0: the default; 0: never; 1 .. 8 mean 9), s_req: MLHIP_MSM_BATCH_BUCKET_SLICE (<= 0:
// the plan's own).  The plan's S is the largest power of two between SLICE_MIN and SLICE_MAX that still gives
// MSM_BATCH_BUCKET_WAVES (slice, window) waves -- long slices mean fuller buckets, so fewer lanes of a wave wait for the
// longest one and the 12 additions of the reduction are shared by more pairs -- and SLICE_MIN where the batch is too small
// for that.  A fixed S is raised to P + 1: a slice is a row with count > P.
inline MsmBatchBucketPlan msm_batch_bucket_plan(const uint64_t* offsets, size_t k, int P, int W, long t_req, long s_req,
                                                const MsmBatchBucketTuning& tune) {
  MsmBatchBucketPlan plan = {tune.min_default, tune.slice_min};
  if (t_req >= 0) plan.T = t_req > 0xffffffffL ? 0xffffffffu : (uint32_t)t_req;
  if (plan.T && plan.T < MSM_BATCH_BUCKET_MIN_FLOOR) plan.T = MSM_BATCH_BUCKET_MIN_FLOOR;
  if (!plan.T) return plan;
  if (s_req > 0) {
    plan.S = s_req > 0x40000000L ? 0x40000000u : (uint32_t)s_req;
    if (plan.S <= (uint32_t)P) plan.S = (uint32_t)P + 1;
    return plan;
  }
  for (uint32_t S = tune.slice_max; S > tune.slice_min; S /= 2) {
    uint64_t slices = 0;
    for (size_t s = 0; s < k; s++) {
      const uint64_t m = offsets[s + 1] - offsets[s];
      if (m >= plan.T) slices += (m + S - 1) / S;
    }
    if (slices * (uint64_t)W >= tune.waves) {
      plan.S = S;
      break;
    }
  }
  return plan;
}
// G1's tuning
inline MsmBatchBucketPlan msm_batch_bucket_plan(const uint64_t* offsets, size_t k, int P, int W, long t_req, long s_req) {
  return msm_batch_bucket_plan(offsets, k, P, W, t_req, s_req, MsmBucketShape<true>::tuning());
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
// past the slice's end write the zero bytes the 16-byte scan reads.  scalars = the slice's first scalar.  WIDTH = the digit
// width of the group (magnitudes 1 .. 2^(WIDTH - 1)).
template <class C, int WIDTH = MSM_BATCH_BUCKET_C>
MLHIP_HD void msm_bucket_digits(uint8_t* rows, uint32_t row_bytes, uint32_t j, uint32_t count, const uint32_t* scalars, bool mont) {
  const WinLayout l = msm_win_layout(C::FR_BITS, WIDTH);
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

// Where pair j of a row's points lies: in the call's own points (mlhip_msm_batch*), or among the bases of a handle through the
// call's index list (mlhip_bases_msm_batch*: index == nullptr means pair j of a segment takes base j, and base0 is the
// position of the row's first pair in its segment).
struct MsmBucketDirect {
  MLHIP_HD size_t operator()(const MsmBatchChunk& ch, uint32_t j) const { return (size_t)ch.first + j; }
};
struct MsmBucketIndexed {
  const uint32_t* index;
  MLHIP_HD size_t operator()(const MsmBatchChunk& ch, uint32_t j) const { return index ? index[ch.first + j] : ch.base0 + j; }
};

// ---- reduction ---------------------------------------------------------------------------------------------------------
constexpr int MSM_BATCH_BUCKET_REDUCE_STEPS = 12;
// One step of the 64-lane reduction, run by every lane: v += the v of lane + d (infinity beyond lane 63), d = 2^(step mod 6).
// neighbour(q, v, d) fetches that value as it was before the step.  After steps 0 .. 5 lane b holds B_b + .. + B_63, after
// steps 6 .. 11 lane 0 holds their sum = sum_b (b + 1) B_b.  LOG = 5: the 32 lane pairs of G2, ten steps, d in pairs.
template <class F, class Ops, int LOG = MSM_BATCH_BUCKET_C - 1, class Neighbour>
MLHIP_HD void msm_bucket_reduce_step(XYZZ<F>& v, int step, Neighbour neighbour) {
  XYZZ<F> q;
  neighbour(q, v, 1u << (step % LOG));
  Ops::add(v, q);
}

// ---- window combination ------------------------------------------------------------------------------------------------
// acc = sum_w 2^off(w) S_w, load(q, w) reading the window sum S_w: Horner from the top window down
template <class F, class Ops, int WIDTH = MSM_BATCH_BUCKET_C, class Load>
MLHIP_HD void msm_bucket_combine(XYZZ<F>& acc, int fr_bits, Load load) {
  const WinLayout l = msm_win_layout(fr_bits, WIDTH);
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
// the same with the digit width as a parameter (G2: 6)
template <class C, int WIDTH>
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
  msm_bucket_digits<C, WIDTH>(digits + (size_t)i * W * row_bytes, row_bytes, j, ch.count, scalars + 8 * ch.first, mont != 0);
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

// The same wave for the two newer uses: G2 (lane pair b owns bucket b, one Fp2 component per lane) and points read through
// an index list (at = MsmBucketIndexed: the table-free path of mlhip_bases_msm_batch*).  LANES_PER = 1: G1, FL = FpField<C>;
// 2: G2, FL = Fp2LField<C>.  Both lanes of a pair scan the same row for the same magnitude, so they load, add and branch
// together (the Fp2 product exchanges components inside the pair).  The reduction moves a value down by d buckets =
// LANES_PER d lanes: every lane receives its own component.  (k_msm_bucket_accumulate above is this body for G1 and the
// call's own points; it stays as it was so that its code object does.)
template <class C, class FL, int LANES_PER, class Ops, class Load>
__device__ __forceinline__ void msm_bucket_wave(XYZZ<FL>& v, const uint8_t* row, uint32_t n16, Load load) {
  typedef MsmBucketShape<LANES_PER == 1> Shape;
  constexpr int WORDS = (int)(sizeof(XYZZ<FL>) / sizeof(uint32_t));
  const uint32_t bucket = threadIdx.x / (uint32_t)LANES_PER;
  msm_bucket_lane<FL>(v, row, n16, bucket, load);
  XYZZ<FL> inf;
  xyzz_set_inf<FL>(inf);
#pragma unroll 1
  for (int step = 0; step < Shape::STEPS; step++)
    msm_bucket_reduce_step<FL, Ops, Shape::LOG>(v, step, [&](XYZZ<FL>& q, const XYZZ<FL>& mine, uint32_t d) {
      const uint32_t* a = reinterpret_cast<const uint32_t*>(&mine);
      const uint32_t* z = reinterpret_cast<const uint32_t*>(&inf);
      uint32_t* b = reinterpret_cast<uint32_t*>(&q);
      const bool beyond = bucket + d >= Shape::BUCKETS;
#pragma unroll
      for (int t = 0; t < WORDS; t++) {
        const uint32_t x = (uint32_t)__shfl_down((int)a[t], (uint32_t)LANES_PER * d, 64);
        b[t] = beyond ? z[t] : x;
      }
    });
}

// G1 over the bases of a handle: pair j of the slice is points[at(row, j)]
template <class C, class At>
__global__ void __launch_bounds__(64) k_msm_bucket_accumulate_at(const Affine<FpField<C>>* __restrict__ points, At at,
                                                                 const MsmBatchChunk* __restrict__ chunks,
                                                                 const uint32_t* __restrict__ slice_rows, uint32_t row_bytes,
                                                                 int W, const uint8_t* __restrict__ digits,
                                                                 XYZZ<FpField<C>>* __restrict__ window_sums) {
  typedef FpField<C> F;
  const uint32_t i = blockIdx.x / (uint32_t)W, w = blockIdx.x % (uint32_t)W;
  const MsmBatchChunk ch = chunks[slice_rows[i]];
  XYZZ<F> v;
  msm_bucket_wave<C, F, 1, MsmBucketOps<F>>(v, digits + ((size_t)i * W + w) * row_bytes, msm_bucket_pad16(ch.count),
                                            [&](Affine<F>& p, uint32_t j) { p = points[at(ch, j)]; });
  if (threadIdx.x == 0) window_sums[(size_t)i * W + w] = v;
}

// G2, one wave per (slice, window); at = MsmBucketDirect (the call's points) or MsmBucketIndexed (a handle's)
template <class C, class At>
__global__ void __launch_bounds__(64) k_msm_bucket_accumulate_lp(const Affine<Fp2Field<C>>* __restrict__ points, At at,
                                                                 const MsmBatchChunk* __restrict__ chunks,
                                                                 const uint32_t* __restrict__ slice_rows, uint32_t row_bytes,
                                                                 int W, const uint8_t* __restrict__ digits,
                                                                 XYZZ<Fp2Field<C>>* __restrict__ window_sums) {
  typedef Fp2LField<C> FL;
  const uint32_t i = blockIdx.x / (uint32_t)W, w = blockIdx.x % (uint32_t)W;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchChunk ch = chunks[slice_rows[i]];
  XYZZ<FL> v;
  msm_bucket_wave<C, FL, 2, MsmBatchOpsLp<C>>(v, digits + ((size_t)i * W + w) * row_bytes, msm_bucket_pad16(ch.count),
                                              [&](Affine<FL>& p, uint32_t j) { lp_load_affine<C>(p, points, at(ch, j), hi); });
  if ((threadIdx.x >> 1) == 0) lp_store_xyzz<C>(window_sums, (size_t)i * W + w, v, hi);
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
// G2: one lane pair per slice
template <class C>
__global__ void __launch_bounds__(64) k_msm_bucket_combine_lp(const XYZZ<Fp2Field<C>>* __restrict__ window_sums,
                                                              const uint32_t* __restrict__ slice_rows, uint32_t n_slices, int W,
                                                              XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (i >= n_slices) return;
  const int hi = (int)(threadIdx.x & 1u);
  XYZZ<FL> acc;
  msm_bucket_combine<FL, MsmBatchOpsLp<C>, MSM_BATCH_BUCKET_C_G2>(
      acc, C::FR_BITS, [&](XYZZ<FL>& q, int w) { lp_load_xyzz<C>(q, window_sums, (size_t)i * W + w, hi); });
  lp_store_xyzz<C>(partials, slice_rows[i], acc, hi);
}

inline long msm_batch_env_long(const char* name) {
  const char* e = getenv(name);
  if (!e || !*e) return -1;
  const long v = atol(e);
  return v < 0 ? -1 : v;
}

// The rows of a call under the switches and the group's tuning, and the geometry of its bucket kernels.
template <class C, class F>
struct MsmBucketCall {
  typedef MsmBucketShape<std::is_same<F, FpField<C>>::value> Shape;
  MsmBatchLayout L;
  std::vector<uint32_t> slices;  // the rows the bucket kernels write; empty: chunks for every segment
  uint32_t n_slices = 0, row_bytes = 0, blocks_per_slice = 0;
  int W = 0;
  size_t digit_bytes = 0, scratch = 0;

  // false: more than 2^32 - 1 rows.  slices stays empty where the route is off, no segment is long, or the scratch or a
  // grid would pass its bound -- L is then msm_batch_layout's.
  bool plan(const uint64_t* offsets, size_t k, int P) {
    W = msm_win_layout(C::FR_BITS, Shape::WIDTH).W;
    const MsmBatchBucketPlan pl = msm_batch_bucket_plan(offsets, k, P, W, msm_batch_env_long("MLHIP_MSM_BATCH_BUCKET_MIN"),
                                                        msm_batch_env_long("MLHIP_MSM_BATCH_BUCKET_SLICE"), Shape::tuning());
    if (!msm_batch_bucket_layout(L, slices, offsets, k, P, pl)) return false;
    if (slices.empty()) return true;
    n_slices = (uint32_t)slices.size();
    uint32_t longest = 0;  // <= S; shorter where every long segment is
    for (uint32_t c : slices) longest = L.chunks[c].count > longest ? L.chunks[c].count : longest;
    row_bytes = msm_bucket_pad16(longest);
    blocks_per_slice = (row_bytes + 63u) / 64u;
    digit_bytes = ((size_t)n_slices * msm_bucket_digit_stride(longest, W) + 255) & ~(size_t)255;
    scratch = digit_bytes + (size_t)n_slices * W * sizeof(XYZZ<F>);
    if (scratch > MSM_BATCH_BUCKET_SCRATCH_MAX || (uint64_t)n_slices * blocks_per_slice >= ((uint64_t)1 << 31) ||
        (uint64_t)n_slices * (uint64_t)W >= ((uint64_t)1 << 31)) {
      slices.clear();
      return msm_batch_layout(L, offsets, k, P);
    }
    return true;
  }

  // digits, accumulate, combine of the slices on st; at = MsmBucketDirect (d_points: the call's) or MsmBucketIndexed (a handle's)
  template <class At>
  void launch(const void* d_points, At at, const void* d_scalars, int mont, const MsmBatchChunk* d_chunks, const uint32_t* d_rows,
              void* part, void* d_scratch, hipStream_t st) const {
    uint8_t* d_digits = (uint8_t*)d_scratch;
    XYZZ<F>* d_wsums = (XYZZ<F>*)((char*)d_scratch + digit_bytes);
    if constexpr (std::is_same<F, FpField<C>>::value) {
      k_msm_bucket_digits<C><<<dim3(n_slices * blocks_per_slice), dim3(64), 0, st>>>(
          (const uint32_t*)d_scalars, mont, d_chunks, d_rows, n_slices, blocks_per_slice, row_bytes, W, d_digits);
      if constexpr (std::is_same<At, MsmBucketDirect>::value)
        k_msm_bucket_accumulate<C><<<dim3(n_slices * (uint32_t)W), dim3(64), 0, st>>>(
            (const Affine<F>*)d_points, d_chunks, d_rows, row_bytes, W, d_digits, d_wsums);
      else
        k_msm_bucket_accumulate_at<C, At><<<dim3(n_slices * (uint32_t)W), dim3(64), 0, st>>>(
            (const Affine<F>*)d_points, at, d_chunks, d_rows, row_bytes, W, d_digits, d_wsums);
      k_msm_bucket_combine<C><<<dim3((n_slices + 63) / 64), dim3(64), 0, st>>>(d_wsums, d_rows, n_slices, W, (XYZZ<F>*)part);
    } else {
      k_msm_bucket_digits<C, Shape::WIDTH><<<dim3(n_slices * blocks_per_slice), dim3(64), 0, st>>>(
          (const uint32_t*)d_scalars, mont, d_chunks, d_rows, n_slices, blocks_per_slice, row_bytes, W, d_digits);
      k_msm_bucket_accumulate_lp<C, At><<<dim3(n_slices * (uint32_t)W), dim3(64), 0, st>>>(
          (const Affine<F>*)d_points, at, d_chunks, d_rows, row_bytes, W, d_digits, d_wsums);
      k_msm_bucket_combine_lp<C><<<dim3((unsigned)((2 * (size_t)n_slices + 63) / 64)), dim3(64), 0, st>>>(d_wsums, d_rows, n_slices,
                                                                                                        W, (XYZZ<F>*)part);
    }
  }
};

// mlhip_msm_batch_device behind the ABI: segments of at least T pairs through the bucket kernels, everything else (a call
// without a long segment, a call whose scratch would pass the bound) as msm_batch_device has it.  subgroup: the points are
// promised to be in G1 / G2 -- the Straus chunks take the split kernels of msm_batch_endo.h, the bucket route stays as it is.
template <class C, class F>
int msm_batch_route_device(const void* d_points, const void* d_scalars, int mont, const uint64_t* offsets, size_t k, void* d_out,
                           hipStream_t st, bool subgroup = false) {
  const int P = msm_batch_chunk_len<C, F>();
  MsmBucketCall<C, F> call;
  if (!call.plan(offsets, k, P)) return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: more than 2^32 - 1 chunks");
  if (call.slices.empty()) return msm_batch_device<C, F>(d_points, d_scalars, mont, offsets, k, d_out, st, subgroup);
  return msm_batch_run<C, F>(
      call.L, call.slices.data(), call.slices.size() * sizeof(uint32_t), d_out, st,
      [&](const MsmBatchChunk* d_chunks, uint32_t n_chunks, const void* d_extra, void* part, void* d_scratch) {
        if (n_chunks > call.n_slices) msm_batch_launch_chunks_p<C, F>(P, d_points, d_scalars, mont, d_chunks, n_chunks, part, st, subgroup);
        call.launch(d_points, MsmBucketDirect(), d_scalars, mont, d_chunks, (const uint32_t*)d_extra, part, d_scratch, st);
      },
      call.scratch);
}
#endif  // __HIPCC__

}  // namespace mlhip
