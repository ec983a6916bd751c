// msm_accumulate.h -- bucket accumulation.  The boundary-form kernels on 32-bit Montgomery limbs (k_accumulate,
// k_big_slices: the second implementation the parity tests compare with, and the slices of plain plans) and the three
// steps of the carry-free accumulation written once over a bucket form (accumulate_seg_body, big_slices_body,
// accumulate_big_body; "bucket forms" below) with the G1 Weierstrass form and its kernels, the quad-lane kernel of small
// MSMs among them.  The Edwards form is in msm_ed.h, the two G2 forms are in msm_g2.h.  Part of msm_kernels.h.
#pragma once
// (included by msm_kernels.h after its common headers, its constants and msm_reduce.h: the LDS trees, the out-of-line group
// operations and the quad loads / stores are there)

namespace mlhip {

template <class F>
__global__ void __launch_bounds__(256) k_accumulate(const Affine<F>* __restrict__ points,
                                                    const uint32_t* __restrict__ sorted,
                                                    const uint32_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ counts, size_t n_buckets,
                                                    const uint32_t* __restrict__ order, uint32_t big_threshold,
                                                    uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
                                                    XYZZ<F>* __restrict__ buckets) {
  size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= n_buckets) return;
  const size_t g = order[tid];  // buckets sorted by population: a wave's lanes run equally long loops
  uint32_t cnt = counts[g];
  if (cnt > big_threshold) {
    uint32_t pos = atomicAdd(big_count, 1u);
    big_list[pos] = (uint32_t)g;
    return;
  }
  XYZZ<F> acc;
  xyzz_set_inf<F>(acc);
  size_t begin = offsets[g];
  msm_accumulate_range<F>(acc, points, sorted, begin, begin + cnt, 1);
  buckets[g] = acc;
}

// ---- G1 accumulation in the carry-free 28-bit-limb form (fp28.h / ec28.h) -------------------------------------
// k_points_to28 rewrites the n input points once per MSM (2 products per point); k_accumulate28_seg is k_accumulate on
// that copy: ~14 % more mixed additions per second because a limb product is one v_mad_i64_i32 with no v_addc and
// field additions carry nothing.
template <class C>
__global__ void __launch_bounds__(256) k_points_to28(const Affine<FpField<C>>* __restrict__ points, size_t n,
                                                     Affine28<C>* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine28<C> q;
  affine28_from<C>(q, points[i]);
  out[i] = q;
}

// ---- long buckets (skewed scalars: small values, equal values, plain sums of points) ---------------------------
// A bucket above the threshold is cut into slices of BIG_SLICE entries; k_big_slices sums every slice with one
// workgroup (so one bucket holding all n points still fills the GPU: 2^20 entries = 256 slices), the combine kernels
// (k_accumulate_big_seg and its G2 / Edwards forms) add the slice sums of a bucket and store / fold the result.
constexpr uint32_t BIG_SLICE = 4096;

// prefix[i] = number of slices of the long buckets before entry i of big_list; prefix[nbig] = total
static __global__ void __launch_bounds__(1024) k_big_prefix(const uint32_t* __restrict__ counts,
                                                            const uint32_t* __restrict__ big_list,
                                                            const uint32_t* __restrict__ big_count,
                                                            uint32_t* __restrict__ prefix) {
  __shared__ uint32_t part[1024];
  __shared__ uint32_t base;
  const uint32_t nbig = *big_count, tid = threadIdx.x;
  if (tid == 0) base = 0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < nbig; c0 += 1024) {
    const uint32_t i = c0 + tid;
    const uint32_t v = i < nbig ? (counts[big_list[i]] + BIG_SLICE - 1) / BIG_SLICE : 0u;
    part[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      const uint32_t t = tid >= d ? part[tid - d] : 0u;
      __syncthreads();
      part[tid] += t;
      __syncthreads();
    }
    if (i < nbig) prefix[i] = base + part[tid] - v;
    __syncthreads();
    if (tid == 1023) base += part[1023];
    __syncthreads();
  }
  if (tid == 0) prefix[nbig] = base;
}

template <class F, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_big_slices(const Affine<F>* __restrict__ points,
                                                      const uint32_t* __restrict__ sorted,
                                                      const uint32_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ counts,
                                                      const uint32_t* __restrict__ big_list,
                                                      const uint32_t* __restrict__ big_count,
                                                      const uint32_t* __restrict__ prefix, XYZZ<F>* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  XYZZ<F>* sh = reinterpret_cast<XYZZ<F>*>(smem);
  __shared__ uint32_t s_bi;
  const uint32_t nbig = *big_count;
  if (nbig == 0) return;
  const uint32_t total = prefix[nbig];
  for (uint32_t sid = blockIdx.x; sid < total; sid += gridDim.x) {
    if (threadIdx.x == 0) {  // the bucket this slice belongs to: last entry with prefix <= sid
      uint32_t lo = 0, hi = nbig - 1;
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= sid)
          lo = mid;
        else
          hi = mid - 1;
      }
      s_bi = lo;
    }
    __syncthreads();
    const uint32_t bi = s_bi;
    const uint32_t g = big_list[bi];
    const size_t first = offsets[g], last = first + counts[g];
    const size_t begin = first + (size_t)(sid - prefix[bi]) * BIG_SLICE;
    const size_t end = begin + BIG_SLICE < last ? begin + BIG_SLICE : last;
    XYZZ<F> acc;
    xyzz_set_inf<F>(acc);
    msm_accumulate_range<F>(acc, points, sorted, begin + threadIdx.x, end, BLOCK);
    block_tree_sum_auto<F, BLOCK>(sh, acc);
    if (threadIdx.x == 0) partials[sid] = sh[0];
    __syncthreads();
  }
}

// sum of the slice sums of long bucket number bi, valid on thread 0 (all threads must call)
template <class F, int BLOCK>
__device__ void big_bucket_total(XYZZ<F>& sum, XYZZ<F>* sh, const XYZZ<F>* __restrict__ partials,
                                 const uint32_t* __restrict__ prefix, uint32_t bi) {
  const uint32_t s0 = prefix[bi], s1 = prefix[bi + 1];
  if (s1 - s0 == 1) {  // the usual case: a bucket just above the threshold
    if (threadIdx.x == 0) sum = partials[s0];
    return;
  }
  XYZZ<F> acc;
  xyzz_set_inf<F>(acc);
  for (uint32_t k = s0 + threadIdx.x; k < s1; k += BLOCK) xyzz_add_ool<F>(acc, partials[k]);
  block_tree_sum_auto<F, BLOCK>(sh, acc);
  if (threadIdx.x == 0) sum = sh[0];
  __syncthreads();
}

// ---- segmented accumulation (host-buffer MSMs streamed over PCIe, plan_stream_train below) --------------------------
// The n pairs arrive in K segments; every segment is sorted by itself and added INTO the bucket sums of the segments
// before it, so the upload of segment s+1 runs under the kernels of segment s and the reduction runs once.  Between
// segments a bucket is kept as its raw carry-free accumulator (4 normalized coordinates; ZZ = 0 limbs <=> infinity),
// which makes the chain of additions identical to the unsegmented kernel's; the last segment writes the boundary form.
#define MLHIP_SEG_FIRST 1
#define MLHIP_SEG_LAST 2
#define MLHIP_SEG_KEEP28 4  // the last segment leaves the raw accumulators too: the reduction reads them (k_chunks_q28)

// ---- bucket forms ---------------------------------------------------------------------------------------------------
// The three steps below are written once over a form Fm, which is the only place that knows how a bucket is kept and
// added to.  A form has LANES lanes per bucket (1, or 2 for G2: `hi` is the lane's place in its pair, and every branch of
// the bodies is pair-uniform) and supplies, per lane:
//   RowMem / Row, load_row          a point of d_points28 and the part of it a lane holds
//   Acc, set_identity, madd         the accumulator (with its infinity flag where the form has one) and the mixed addition
//   State, load_state, store_state  the accumulator in d_state28 (all-zero limbs <=> infinity where the form has a flag)
//   LaneB, to_boundary, load_lane, store_lane, block_sum   the lane's part of a boundary-form XYZZ<BF>, in d_buckets /
//                                   partials / LDS, and the LDS tree over a workgroup's lanes (quads for one-lane forms,
//                                   lane pairs for G2); HAS_BOUNDARY = false: the buckets of this form never leave
//                                   through d_buckets (Edwards)
//   state_to_boundary, boundary_to_state   whole buckets on one thread, for the combine of long buckets; the first
//                                   returns false when there is nothing to add
// Forms: G1Form28 (below), EdForm28 (msm_ed.h), G2Form28 and G2KcForm28 (msm_g2.h).

// One segment's entries into the buckets, one bucket per LANES lanes.  With FIRST | LAST and no KEEP28 (a one-pass plan
// whose reduction reads the boundary form) `state` is neither read nor written and may be null.
template <class Fm>
__device__ __forceinline__ void accumulate_seg_body(const typename Fm::RowMem* __restrict__ rows,
                                                    const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ counts, size_t n_buckets,
                                                    const uint32_t* __restrict__ order, uint32_t big_threshold,
                                                    uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
                                                    typename Fm::State* __restrict__ state, int flags,
                                                    XYZZ<typename Fm::BF>* __restrict__ buckets) {
  const size_t slot = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / Fm::LANES;
  if (slot >= n_buckets) return;
  const int hi = (int)(threadIdx.x % Fm::LANES);
  const size_t g = order[slot];  // buckets sorted by population: a wave's lanes run equally long loops
  const uint32_t cnt = counts[g];
  const bool first = (flags & MLHIP_SEG_FIRST) != 0, last = (flags & MLHIP_SEG_LAST) != 0;
  if (cnt > big_threshold) {  // the combine kernel adds this segment's entries to the bucket's state
    if (!hi) {
      uint32_t pos = atomicAdd(big_count, 1u);
      big_list[pos] = (uint32_t)g;
    }
    return;
  }
  const bool to_boundary = Fm::HAS_BOUNDARY && last && !(flags & MLHIP_SEG_KEEP28);
  if (cnt == 0 && !first && !to_boundary) return;  // nothing to add, nothing to convert
  typename Fm::Acc acc;
  if (first)
    Fm::set_identity(acc);
  else
    Fm::load_state(acc, state, g, hi);
  const size_t begin = offsets[g], end = begin + cnt;
  if (cnt != 0) {
    uint32_t e = sorted[begin];
    typename Fm::Row p;
    Fm::load_row(p, rows, e & 0x7fffffffu, hi);
    for (size_t k = begin; k < end; k++) {
      uint32_t en = e;
      typename Fm::Row pn = p;
      if (k + 1 < end) {  // prefetch the next index and point under this addition
        en = sorted[k + 1];
        Fm::load_row(pn, rows, en & 0x7fffffffu, hi);
      }
      Fm::madd(acc, p, (e >> 31) != 0);
      e = en;
      p = pn;
    }
  }
  if constexpr (Fm::HAS_BOUNDARY) {
    if (to_boundary) {
      typename Fm::LaneB r;
      Fm::to_boundary(r, acc);
      Fm::store_lane(buckets, g, r, hi);
      return;
    }
  }
  Fm::store_state(state, g, acc, hi);
}

// The slice sums of the long buckets from the carry-free rows (a shifted-base table keeps no boundary-form rows):
// k_big_slices with the form's per-lane loop; a lane's sum goes to the boundary form for the LDS tree, so the partial sums
// have the format the combine reads.
template <class Fm, int BLOCK>
__device__ __forceinline__ void big_slices_body(const typename Fm::RowMem* __restrict__ rows, const uint32_t* __restrict__ sorted,
                                                const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
                                                const uint32_t* __restrict__ big_list, const uint32_t* __restrict__ big_count,
                                                const uint32_t* __restrict__ prefix,
                                                XYZZ<typename Fm::BF>* __restrict__ partials) {
  typedef XYZZ<typename Fm::BF> X;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  X* sh = reinterpret_cast<X*>(smem);
  __shared__ uint32_t s_bi;
  constexpr uint32_t UNITS = BLOCK / Fm::LANES;
  const uint32_t uid = threadIdx.x / Fm::LANES;
  const int hi = (int)(threadIdx.x % Fm::LANES);
  const uint32_t nbig = *big_count;
  if (nbig == 0) return;
  const uint32_t total = prefix[nbig];
  for (uint32_t sid = blockIdx.x; sid < total; sid += gridDim.x) {
    if (threadIdx.x == 0) {  // the bucket this slice belongs to: last entry with prefix <= sid
      uint32_t lo = 0, up = nbig - 1;
      while (lo < up) {
        const uint32_t mid = (lo + up + 1) >> 1;
        if (prefix[mid] <= sid)
          lo = mid;
        else
          up = mid - 1;
      }
      s_bi = lo;
    }
    __syncthreads();
    const uint32_t bi = s_bi;
    const uint32_t g = big_list[bi];
    const size_t first = offsets[g], last = first + counts[g];
    const size_t begin = first + (size_t)(sid - prefix[bi]) * BIG_SLICE;
    const size_t end = begin + BIG_SLICE < last ? begin + BIG_SLICE : last;
    typename Fm::Acc acc;
    Fm::set_identity(acc);
    for (size_t k = begin + uid; k < end; k += UNITS) {  // pair-uniform bounds
      const uint32_t e = sorted[k];
      typename Fm::Row q;
      Fm::load_row(q, rows, e & 0x7fffffffu, hi);
      Fm::madd(acc, q, (e >> 31) != 0);
    }
    typename Fm::LaneB b;
    Fm::to_boundary(b, acc);
    Fm::template block_sum<BLOCK>(sh, b, hi);
    if (uid == 0) {
      Fm::load_lane(b, sh, 0, hi);
      Fm::store_lane(partials, sid, b, hi);
    }
    __syncthreads();
  }
}

// The long buckets of a segment: total of the slice sums (boundary form), then state <- state + total, or the boundary
// form on the last segment of a plan that reduces from it (thread 0)
template <class Fm, int BLOCK>
__device__ __forceinline__ void accumulate_big_body(const uint32_t* __restrict__ big_list, const uint32_t* __restrict__ big_count,
                                                    const uint32_t* __restrict__ prefix,
                                                    const XYZZ<typename Fm::BF>* __restrict__ partials,
                                                    typename Fm::State* __restrict__ state, int flags,
                                                    XYZZ<typename Fm::BF>* __restrict__ buckets) {
  typedef typename Fm::BF F;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  XYZZ<F>* sh = reinterpret_cast<XYZZ<F>*>(smem);
  const uint32_t nbig = *big_count;
  const bool first = (flags & MLHIP_SEG_FIRST) != 0;
  const bool to_boundary = Fm::HAS_BOUNDARY && (flags & MLHIP_SEG_LAST) != 0 && !(flags & MLHIP_SEG_KEEP28);
  for (uint32_t bi = blockIdx.x; bi < nbig; bi += gridDim.x) {
    const uint32_t g = big_list[bi];
    XYZZ<F> sum;
    big_bucket_total<F, BLOCK>(sum, sh, partials, prefix, bi);
    if (threadIdx.x == 0) {
      if (!first) {
        XYZZ<F> prev;
        if (Fm::state_to_boundary(prev, state, g)) xyzz_add_ool<F>(sum, prev);
      }
      if (to_boundary)
        buckets[g] = sum;
      else
        Fm::boundary_to_state(state, g, sum);
    }
    __syncthreads();
  }
}

// ---- the G1 Weierstrass form: Affine28 rows, XYZZ28 accumulators (ec28.h) ---------------------------------------------
template <class C>
MLHIP_HD void xyzz28_zero(XYZZ28<C>& r) {  // the state of an empty bucket
  fp28_zero<C>(r.x);
  fp28_zero<C>(r.y);
  fp28_zero<C>(r.zz);
  fp28_zero<C>(r.zzz);
}

template <class C>
struct G1Form28 {
  static constexpr int LANES = 1;
  static constexpr bool HAS_BOUNDARY = true;
  typedef FpField<C> BF;
  typedef Affine28<C> RowMem, Row;
  typedef XYZZ28<C> State;
  typedef XYZZ<BF> LaneB;
  struct Acc {
    XYZZ28<C> p;
    bool inf;
  };
  static __device__ __forceinline__ void load_row(Row& r, const RowMem* rows, uint32_t i, int) { r = rows[i]; }
  MLHIP_HD static void set_identity(Acc& a) { a.inf = true; }
  MLHIP_HD static void madd(Acc& a, const Row& q, bool negate) { xyzz28_madd<C>(a.p, a.inf, q, negate); }
  static __device__ __forceinline__ void load_state(Acc& a, const State* state, size_t g, int) {
    a.p = state[g];
    a.inf = fp28_all_zero<C>(a.p.zz);
  }
  static __device__ __forceinline__ void store_state(State* state, size_t g, Acc& a, int) {
    if (a.inf) xyzz28_zero<C>(a.p);
    state[g] = a.p;
  }
  MLHIP_HD static void to_boundary(LaneB& r, const Acc& a) { xyzz28_to<C>(r, a.p, a.inf); }
  static __device__ __forceinline__ void load_lane(LaneB& r, const XYZZ<BF>* src, size_t i, int) { r = src[i]; }
  static __device__ __forceinline__ void store_lane(XYZZ<BF>* dst, size_t i, const LaneB& r, int) { dst[i] = r; }
  template <int BLOCK>
  static __device__ __forceinline__ void block_sum(XYZZ<BF>* sh, const LaneB& mine, int) {
    block_tree_sum_auto<BF, BLOCK>(sh, mine);
  }
  static __device__ __forceinline__ bool state_to_boundary(XYZZ<BF>& r, const State* state, size_t g) {
    const XYZZ28<C> s28 = state[g];
    xyzz28_to<C>(r, s28, fp28_all_zero<C>(s28.zz));
    return true;
  }
  static __device__ __forceinline__ void boundary_to_state(State* state, size_t g, const XYZZ<BF>& sum) {
    XYZZ28<C> s28;
    if (xyzz_is_inf<BF>(sum)) {
      xyzz28_zero<C>(s28);
    } else {
      fp28_from_fp<C>(s28.x, sum.x);
      fp28_from_fp<C>(s28.y, sum.y);
      fp28_from_fp<C>(s28.zz, sum.zz);
      fp28_from_fp<C>(s28.zzz, sum.zzz);
    }
    state[g] = s28;
  }
};

template <class C>
__global__ void __launch_bounds__(256) k_accumulate28_seg(const Affine28<C>* __restrict__ points,
                                                          const uint32_t* __restrict__ sorted,
                                                          const uint32_t* __restrict__ offsets,
                                                          const uint32_t* __restrict__ counts, size_t n_buckets,
                                                          const uint32_t* __restrict__ order, uint32_t big_threshold,
                                                          uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
                                                          XYZZ28<C>* __restrict__ state, int flags,
                                                          XYZZ<FpField<C>>* __restrict__ buckets) {
  accumulate_seg_body<G1Form28<C>>(points, sorted, offsets, counts, n_buckets, order, big_threshold, big_list, big_count, state,
                                   flags, buckets);
}

template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_accumulate_big_seg(const uint32_t* __restrict__ big_list,
                                                              const uint32_t* __restrict__ big_count,
                                                              const uint32_t* __restrict__ prefix,
                                                              const XYZZ<FpField<C>>* __restrict__ partials,
                                                              XYZZ28<C>* __restrict__ state, int flags,
                                                              XYZZ<FpField<C>>* __restrict__ buckets) {
  accumulate_big_body<G1Form28<C>, BLOCK>(big_list, big_count, prefix, partials, state, flags, buckets);
}

// Bucket accumulation with one bucket per QUAD of lanes, for MSMs too small to fill the chip with one lane per bucket:
// what such an MSM waits for is the chain of dependent additions of its fullest bucket, and on a quad an addition is four
// rounds of one product per lane (quad28_xyzz_add; the point enters as (x, +-y, 1, 1)) instead of ten products in a row.
// Leaves the carry-free bucket state the reduction reads (as k_accumulate28_seg with MLHIP_SEG_KEEP28).
template <class C>
__global__ void __launch_bounds__(256) k_accumulate_q28(const Affine28<C>* __restrict__ points,
                                                        const uint32_t* __restrict__ sorted,
                                                        const uint32_t* __restrict__ offsets,
                                                        const uint32_t* __restrict__ counts, size_t n_buckets,
                                                        uint32_t big_threshold, uint32_t* __restrict__ big_list,
                                                        uint32_t* __restrict__ big_count, XYZZ28<C>* __restrict__ state) {
  typedef QuadDevice28<C> B;
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (g >= n_buckets) return;  // quad-uniform
  const unsigned lane = threadIdx.x & 3u;
  const uint32_t cnt = counts[g];
  if (cnt > big_threshold) {  // k_big_slices / k_accumulate_big_seg write this bucket's state
    if (lane == 0) {
      const uint32_t pos = atomicAdd(big_count, 1u);
      big_list[pos] = (uint32_t)g;
    }
    return;
  }
  Fp28<C> acc, one;
  fp28_zero<C>(acc);
  fp28_from_const<C>(one, C::ONE28);
  const size_t begin = offsets[g], end = begin + cnt;
#pragma unroll 1
  for (size_t k = begin; k < end; k++) {
    const uint32_t e = sorted[k];
    const Fp28<C>* q = reinterpret_cast<const Fp28<C>*>(points + (e & 0x7fffffffu));  // x | y
    Fp28<C> c = q[lane & 1u], n, b;
    // the point at infinity is (0, 0): skip it (quad-uniform: lanes 0 and 1 hold x and y)
    const unsigned z = B::quad_or((fp28_all_zero<C>(c) ? 1u : 0u) << lane);
    if ((z & 3u) == 3u) continue;
    fp28_neg<C>(n, c);
    fp28_select<C>(c, lane == 1 && (e >> 31) != 0, n, c);
    fp28_select<C>(b, lane >= 2, one, c);
    quad28_xyzz_add<C, B>(acc, b);
  }
  quad28_store<C>(state, g, acc);
}

}  // namespace mlhip
