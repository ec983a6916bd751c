// msm_g2.h -- G2 over lane pairs: the boundary-form accumulation and slices (second implementation; slices of plain plans),
// the two carry-free bucket forms (G2Form28, G2KcForm28) with their kernels over the shared bodies of msm_accumulate.h, and
// the two reduction forms (PairForm, Pair28Form) with their kernels over the shared bodies of msm_reduce.h.  Part of
// msm_kernels.h.
#pragma once
// (included by msm_kernels.h after its common headers and constants)

namespace mlhip {

// ---- G2 over lane pairs -----------------------------------------------------------------------------
// A G2 bucket is owned by two adjacent lanes, one Fp2 component each (fp2_lanes.h): the XYZZ accumulator is
// 4 x 12 words per lane -- the G1 footprint -- so the mixed addition stays in registers (one Fp2 element per
// lane needs ~340 live words and spills), and every Fp2 product is one fused dual Montgomery product.
template <class C>
struct Fp2LField {
  using Curve = C;
  using T = Fp2L<C>;
  MLHIP_HD static void zero(T& r) { fp2_zero<C>(r); }
  MLHIP_HD static void one(T& r) { fp2_one<C>(r); }
  MLHIP_HD static bool is_zero(const T& a) { return fp2_is_zero<C>(a); }
  MLHIP_HD static bool eq(const T& a, const T& b) { return fp2_eq<C>(a, b); }
  MLHIP_HD static void add(T& r, const T& a, const T& b) { fp2_add<C>(r, a, b); }
  MLHIP_HD static void sub(T& r, const T& a, const T& b) { fp2_sub<C>(r, a, b); }
  MLHIP_HD static void dbl(T& r, const T& a) { fp2_dbl<C>(r, a); }
  MLHIP_HD static void neg(T& r, const T& a) { fp2_neg<C>(r, a); }
  MLHIP_HD static void mul(T& r, const T& a, const T& b) { fp2_mul<C>(r, a, b); }
  MLHIP_HD static void sqr(T& r, const T& a) { fp2_sqr<C>(r, a); }
  MLHIP_HD static void inv(T& r, const T& a) { fp2_inv<C>(r, a); }
  MLHIP_HD static void select(T& r, bool c, const T& a, const T& b) { fp2_select<C>(r, c, a, b); }
};

// component loads / stores between the AoS Fp2 layout in memory and the lane-pair registers
template <class C>
__device__ __forceinline__ void lp_load_affine(Affine<Fp2LField<C>>& p, const Affine<Fp2Field<C>>* pts, size_t idx, int hi) {
  const Fp<C>* q = reinterpret_cast<const Fp<C>*>(pts + idx);
  p.x.v = q[hi];
  p.y.v = q[2 + hi];
}
template <class C>
__device__ __forceinline__ void lp_load_xyzz(XYZZ<Fp2LField<C>>& r, const XYZZ<Fp2Field<C>>* src, size_t idx, int hi) {
  const Fp<C>* q = reinterpret_cast<const Fp<C>*>(src + idx);
  r.x.v = q[hi];
  r.y.v = q[2 + hi];
  r.zz.v = q[4 + hi];
  r.zzz.v = q[6 + hi];
}
template <class C>
__device__ __forceinline__ void lp_store_xyzz(XYZZ<Fp2Field<C>>* dst, size_t idx, const XYZZ<Fp2LField<C>>& r, int hi) {
  Fp<C>* q = reinterpret_cast<Fp<C>*>(dst + idx);
  q[hi] = r.x.v;
  q[2 + hi] = r.y.v;
  q[4 + hi] = r.zz.v;
  q[6 + hi] = r.zzz.v;
}
template <class C>
__device__ __noinline__ void xyzz_add_lp_ool(XYZZ<Fp2LField<C>>& acc, const XYZZ<Fp2LField<C>>& q) {
  xyzz_add<Fp2LField<C>>(acc, q);
}

// ---- the G2 reduction forms (see "reduction forms", msm_reduce.h) ------------------------------------------------------
// PairForm: one point per lane pair in the boundary form -- the test build's reduction (MLHIP_REDUCE32 / MLHIP_ACC32), the
// combine of folded plans and the tree of the long buckets.
template <class C>
struct PairForm {
  static constexpr int LANES = 2;
  static constexpr bool CHUNK_PREFETCH = false, TREE_HAND_OVER = true;
  typedef Fp2Field<C> BF;
  typedef XYZZ<BF> Mem;
  typedef XYZZ<Fp2LField<C>> V;
  static __device__ __forceinline__ int hi() { return lane_is_hi() ? 1 : 0; }
  static constexpr int MEMS = 1;
  static __device__ __forceinline__ void set_empty(V& v) { xyzz_set_inf<Fp2LField<C>>(v); }
  static __device__ __forceinline__ void load(V& v, const Mem* arr, size_t i) { lp_load_xyzz<C>(v, arr, i, hi()); }
  static __device__ __forceinline__ void store(Mem* arr, size_t i, const V& v) { lp_store_xyzz<C>(arr, i, v, hi()); }
  static __device__ __forceinline__ void add(V& a, const V& b) { xyzz_add_lp_ool<C>(a, b); }
  static __device__ __forceinline__ void store_out(XYZZ<BF>* out, size_t i, const V& v) { store(out, i, v); }
};

// LDS tree over the BLOCK / 2 lane pairs of a workgroup, in the boundary form; the sum is left in sh[0]
template <class C, int BLOCK>
__device__ __forceinline__ void block_tree_sum_lp(XYZZ<Fp2Field<C>>* sh, const XYZZ<Fp2LField<C>>& mine) {
  XYZZ<Fp2LField<C>> acc = mine;
  group_tree_sum<PairForm<C>>(sh, acc, threadIdx.x >> 1, BLOCK / 2);
}

template <class C>
__global__ void __launch_bounds__(256) k_accumulate_lp(const Affine<Fp2Field<C>>* __restrict__ points,
                                                       const uint32_t* __restrict__ sorted,
                                                       const uint32_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ counts, size_t n_buckets,
                                                       const uint32_t* __restrict__ order, uint32_t big_threshold,
                                                       uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
                                                       XYZZ<Fp2Field<C>>* __restrict__ buckets) {
  typedef Fp2LField<C> FL;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t pair = t >> 1;  // both lanes of a pair share the bucket: every branch below is pair-uniform
  if (pair >= n_buckets) return;
  const int hi = lane_is_hi() ? 1 : 0;
  const size_t g = order[pair];
  const uint32_t cnt = counts[g];
  if (cnt > big_threshold) {
    if (!hi) {
      uint32_t pos = atomicAdd(big_count, 1u);
      big_list[pos] = (uint32_t)g;
    }
    return;
  }
  XYZZ<FL> acc;
  xyzz_set_inf<FL>(acc);
  const size_t begin = offsets[g], end = begin + cnt;
  if (begin < end) {
    uint32_t e = sorted[begin];
    Affine<FL> p;
    lp_load_affine<C>(p, points, e & 0x7fffffffu, hi);
    for (size_t k = begin; k < end; k++) {
      uint32_t en = e;
      Affine<FL> pn = p;
      if (k + 1 < end) {
        en = sorted[k + 1];
        lp_load_affine<C>(pn, points, en & 0x7fffffffu, hi);
      }
      xyzz_madd<FL>(acc, p, (e >> 31) != 0);
      e = en;
      p = pn;
    }
  }
  lp_store_xyzz<C>(buckets, g, acc, hi);
}

// ---- slice sums of long G2 buckets over lane pairs (k_big_slices is the one-lane form: ~340 live words per lane) ------
// BLOCK / 2 pairs stride over the slice's entries with the lane-pair mixed addition, then an LDS tree of lane-pair
// additions; slice bookkeeping as in k_big_slices (msm_accumulate.h).
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_big_slices_lp(const Affine<Fp2Field<C>>* __restrict__ points,
                                                         const uint32_t* __restrict__ sorted,
                                                         const uint32_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ big_list,
                                                         const uint32_t* __restrict__ big_count,
                                                         const uint32_t* __restrict__ prefix,
                                                         XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  XYZZ<Fp2Field<C>>* sh = reinterpret_cast<XYZZ<Fp2Field<C>>*>(smem);
  __shared__ uint32_t s_bi;
  constexpr uint32_t PAIRS = BLOCK / 2;
  const uint32_t pid = threadIdx.x >> 1;
  const int hi = lane_is_hi() ? 1 : 0;
  const uint32_t nbig = *big_count;
  if (nbig == 0) return;
  const uint32_t total = prefix[nbig];
  for (uint32_t sid = blockIdx.x; sid < total; sid += gridDim.x) {
    if (threadIdx.x == 0) {
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
    XYZZ<FL> acc;
    xyzz_set_inf<FL>(acc);
    for (size_t k = begin + pid; k < end; k += PAIRS) {  // pair-uniform bounds
      const uint32_t e = sorted[k];
      Affine<FL> q;
      lp_load_affine<C>(q, points, e & 0x7fffffffu, hi);
      xyzz_madd<FL>(acc, q, (e >> 31) != 0);
    }
    block_tree_sum_lp<C, BLOCK>(sh, acc);
    if (pid == 0) {
      XYZZ<FL> a;
      lp_load_xyzz<C>(a, sh, 0, hi);
      lp_store_xyzz<C>(partials, sid, a, hi);
    }
    __syncthreads();
  }
}

// ---- G2 accumulation in the carry-free form over lane pairs (ec28_lp.h; curves with u^2 = -1) -----------------
template <class C>
struct alignas(8) AffineG2_28 {  // x.c0 | x.c1 | y.c0 | y.c1, 56 (40) bytes each
  Fp28<C> c[4];
};

template <class C>
__global__ void __launch_bounds__(256) k_points_to28_g2(const Affine<Fp2Field<C>>* __restrict__ points, size_t n,
                                                        AffineG2_28<C>* __restrict__ out) {
  // one coordinate component per thread: 4 threads per point
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * n) return;
  const Fp<C>* src = reinterpret_cast<const Fp<C>*>(points);
  Fp28<C> v;
  fp28_from_fp<C>(v, src[t]);
  reinterpret_cast<Fp28<C>*>(out)[t] = v;
}

// a bucket's carry-free state: two XYZZ28L, one per lane; ZZ = 0 limbs in both for the point at infinity
template <class C>
__device__ __forceinline__ void lp28_store_state(XYZZ28L<Fp28<C>>* dst, size_t idx, XYZZ28L<Fp28<C>> r, bool inf, int hi) {
  if (inf) {
#pragma unroll
    for (int i = 0; i < C::N28; i++) r.x.l[i] = r.y.l[i] = r.zz.l[i] = r.zzz.l[i] = 0;
  }
  dst[2 * idx + hi] = r;
}

// ---- the G2 bucket forms (see "bucket forms", msm_accumulate.h) ---------------------------------------------------------
// G2Form28: the pair split by component (ec28_lp.h): each lane holds one Fp2 component of the point and of the accumulator,
// every Fp2 product is one fused dual product.
template <class C>
struct G2Form28 {
  static constexpr int LANES = 2;
  static constexpr bool HAS_BOUNDARY = true;
  typedef Fp2Field<C> BF;
  typedef AffineG2_28<C> RowMem;
  typedef Affine28L<Fp28<C>> Row;
  typedef XYZZ28L<Fp28<C>> State;
  typedef XYZZ<Fp2LField<C>> LaneB;
  struct Acc {
    XYZZ28L<Fp28<C>> p;
    bool inf;
  };
  static __device__ __forceinline__ void load_row(Row& r, const RowMem* rows, uint32_t i, int hi) {
    r.x = rows[i].c[hi];
    r.y = rows[i].c[2 + hi];
  }
  MLHIP_HD static void set_identity(Acc& a) { a.inf = true; }
  MLHIP_HD static void madd(Acc& a, const Row& q, bool negate) { xyzz28_lp_madd<C, PairDevice<C>>(a.p, a.inf, q, negate); }
  static __device__ __forceinline__ void load_state(Acc& a, const State* state, size_t g, int hi) {
    a.p = state[2 * g + hi];
    const uint32_t z = fp28_all_zero<C>(a.p.zz) ? 1u : 0u;
    a.inf = (z & pair_xchg_u32(z)) != 0;  // ZZ = 0 in Fp2: both components
  }
  static __device__ __forceinline__ void store_state(State* state, size_t g, const Acc& a, int hi) {
    lp28_store_state<C>(state, g, a.p, a.inf, hi);
  }
  static __device__ __forceinline__ void to_boundary(LaneB& r, const Acc& a) {
    if (a.inf) {
      xyzz_set_inf<Fp2LField<C>>(r);
    } else {
      fp28_to_fp<C>(r.x.v, a.p.x);
      fp28_to_fp<C>(r.y.v, a.p.y);
      fp28_to_fp<C>(r.zz.v, a.p.zz);
      fp28_to_fp<C>(r.zzz.v, a.p.zzz);
    }
  }
  static __device__ __forceinline__ void load_lane(LaneB& r, const XYZZ<BF>* src, size_t i, int hi) {
    lp_load_xyzz<C>(r, src, i, hi);
  }
  static __device__ __forceinline__ void store_lane(XYZZ<BF>* dst, size_t i, const LaneB& r, int hi) {
    lp_store_xyzz<C>(dst, i, r, hi);
  }
  template <int BLOCK>
  static __device__ __forceinline__ void block_sum(XYZZ<BF>* sh, const LaneB& mine, int) {
    block_tree_sum_lp<C, BLOCK>(sh, mine);
  }
  // whole buckets on one thread, for the combine: both lanes' halves
  static __device__ __forceinline__ bool state_to_boundary(XYZZ<BF>& r, const State* state, size_t g) {
    const State lo = state[2 * g], up = state[2 * g + 1];
    if (fp28_all_zero<C>(lo.zz) && fp28_all_zero<C>(up.zz)) return false;
    fp28_to_fp<C>(r.x.c0, lo.x);
    fp28_to_fp<C>(r.x.c1, up.x);
    fp28_to_fp<C>(r.y.c0, lo.y);
    fp28_to_fp<C>(r.y.c1, up.y);
    fp28_to_fp<C>(r.zz.c0, lo.zz);
    fp28_to_fp<C>(r.zz.c1, up.zz);
    fp28_to_fp<C>(r.zzz.c0, lo.zzz);
    fp28_to_fp<C>(r.zzz.c1, up.zzz);
    return true;
  }
  static __device__ __forceinline__ void boundary_to_state(State* state, size_t g, const XYZZ<BF>& sum) {
    State lo, up;
    if (xyzz_is_inf<BF>(sum)) {
#pragma unroll
      for (int i = 0; i < C::N28; i++) {
        lo.x.l[i] = lo.y.l[i] = lo.zz.l[i] = lo.zzz.l[i] = 0;
        up.x.l[i] = up.y.l[i] = up.zz.l[i] = up.zzz.l[i] = 0;
      }
    } else {
      fp28_from_fp<C>(lo.x, sum.x.c0);
      fp28_from_fp<C>(up.x, sum.x.c1);
      fp28_from_fp<C>(lo.y, sum.y.c0);
      fp28_from_fp<C>(up.y, sum.y.c1);
      fp28_from_fp<C>(lo.zz, sum.zz.c0);
      fp28_from_fp<C>(up.zz, sum.zz.c1);
      fp28_from_fp<C>(lo.zzz, sum.zzz.c0);
      fp28_from_fp<C>(up.zzz, sum.zzz.c1);
    }
    state[2 * g] = lo;
    state[2 * g + 1] = up;
  }
};

// G2KcForm28: the pair split by coordinate (ec28_kc.h): lane A (hi = 0) owns X and ZZ, lane B owns Y and ZZZ, every Fp2
// product is a one-lane Karatsuba product.  Rows, state and buckets keep the layouts of G2Form28 -- a lane simply reads both
// components of its two coordinates (state[2 g] holds the real parts {x, y, zz, zzz}, state[2 g + 1] the imaginary parts)
// and the x or the y half of a point (56 + 56 contiguous bytes) -- so the state is bit-identical and the long-bucket kernels
// of G2Form28 serve both.
template <class C>
struct G2KcForm28 : G2Form28<C> {
  typedef Fp2Field<C> BF;
  typedef AffineG2_28<C> RowMem;
  typedef XYZZ28L<Fp28<C>> State;
  typedef Fp2x28<C> Row;
  struct Acc {
    Fp2x28<C> u, z;  // A: X, ZZ   B: Y, ZZZ
    bool inf;
  };
  struct LaneB {
    Fp<C> u0, u1, z0, z1;
  };
  static __device__ __forceinline__ void load_row(Row& r, const RowMem* rows, uint32_t i, int hi) {
    r.c0 = rows[i].c[2 * hi];
    r.c1 = rows[i].c[2 * hi + 1];
  }
  MLHIP_HD static void set_identity(Acc& a) { a.inf = true; }
  MLHIP_HD static void madd(Acc& a, const Row& q, bool negate) { xyzz28_kc_madd<C, KcDevice<C>>(a.u, a.z, a.inf, q, negate); }
  static __device__ __forceinline__ void load_state(Acc& a, const State* state, size_t g, int hi) {
    const Fp28<C>* st = reinterpret_cast<const Fp28<C>*>(state + 2 * g);
    a.u.c0 = st[hi];
    a.u.c1 = st[4 + hi];
    a.z.c0 = st[2 + hi];
    a.z.c1 = st[6 + hi];
    const bool zf[1] = {fp28_all_zero<C>(a.z.c0) && fp28_all_zero<C>(a.z.c1)};
    a.inf = KcDevice<C>::of_a(zf);  // ZZ = 0 in Fp2
  }
  static __device__ __forceinline__ void store_state(State* state, size_t g, Acc& a, int hi) {
    Fp28<C>* st = reinterpret_cast<Fp28<C>*>(state + 2 * g);
    if (a.inf) {
      fp28_zero<C>(a.u.c0);
      fp28_zero<C>(a.u.c1);
      fp28_zero<C>(a.z.c0);
      fp28_zero<C>(a.z.c1);
    }
    st[hi] = a.u.c0;
    st[4 + hi] = a.u.c1;
    st[2 + hi] = a.z.c0;
    st[6 + hi] = a.z.c1;
  }
  static __device__ __forceinline__ void to_boundary(LaneB& r, const Acc& a) {
    if (a.inf) {  // as xyzz_set_inf: X = Y = 1, ZZ = ZZZ = 0
      fp_one<C>(r.u0);
      fp_zero<C>(r.u1);
      fp_zero<C>(r.z0);
      fp_zero<C>(r.z1);
    } else {
      fp28_to_fp<C>(r.u0, a.u.c0);
      fp28_to_fp<C>(r.u1, a.u.c1);
      fp28_to_fp<C>(r.z0, a.z.c0);
      fp28_to_fp<C>(r.z1, a.z.c1);
    }
  }
  static __device__ __forceinline__ void store_lane(XYZZ<BF>* dst, size_t i, const LaneB& r, int hi) {
    Fp<C>* q = reinterpret_cast<Fp<C>*>(dst + i);  // x.c0 x.c1 y.c0 y.c1 zz.c0 zz.c1 zzz.c0 zzz.c1
    q[2 * hi] = r.u0;
    q[2 * hi + 1] = r.u1;
    q[4 + 2 * hi] = r.z0;
    q[5 + 2 * hi] = r.z1;
  }
};

// segmented G2 accumulation (carry-free form; curves with u^2 = -1 may take the coordinate split, test build only)
template <class C>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_accumulate28_lp_seg(
    const AffineG2_28<C>* __restrict__ points, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
    const uint32_t* __restrict__ counts, size_t n_buckets, const uint32_t* __restrict__ order, uint32_t big_threshold,
    uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count, XYZZ28L<Fp28<C>>* __restrict__ state, int flags,
    XYZZ<Fp2Field<C>>* __restrict__ buckets) {
  accumulate_seg_body<G2Form28<C>>(points, sorted, offsets, counts, n_buckets, order, big_threshold, big_list, big_count, state,
                                   flags, buckets);
}

template <class C>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_accumulate28_kc_seg(
    const AffineG2_28<C>* __restrict__ points, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
    const uint32_t* __restrict__ counts, size_t n_buckets, const uint32_t* __restrict__ order, uint32_t big_threshold,
    uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count, XYZZ28L<Fp28<C>>* __restrict__ state, int flags,
    XYZZ<Fp2Field<C>>* __restrict__ buckets) {
  accumulate_seg_body<G2KcForm28<C>>(points, sorted, offsets, counts, n_buckets, order, big_threshold, big_list, big_count,
                                     state, flags, buckets);
}

template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_accumulate_big_seg_g2(const uint32_t* __restrict__ big_list,
                                                                 const uint32_t* __restrict__ big_count,
                                                                 const uint32_t* __restrict__ prefix,
                                                                 const XYZZ<Fp2Field<C>>* __restrict__ partials,
                                                                 XYZZ28L<Fp28<C>>* __restrict__ state, int flags,
                                                                 XYZZ<Fp2Field<C>>* __restrict__ buckets) {
  accumulate_big_body<G2Form28<C>, BLOCK>(big_list, big_count, prefix, partials, state, flags, buckets);
}

// k_big_slices_lp from the carry-free rows of a shifted-base table: BLOCK / 2 lane pairs stride over the slice's entries
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_big_slices_lp28(const AffineG2_28<C>* __restrict__ points,
                                                           const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ big_list,
                                                           const uint32_t* __restrict__ big_count,
                                                           const uint32_t* __restrict__ prefix,
                                                           XYZZ<Fp2Field<C>>* __restrict__ partials) {
  big_slices_body<G2Form28<C>, BLOCK>(points, sorted, offsets, counts, big_list, big_count, prefix, partials);
}

// ---- the G2 reduction ------------------------------------------------------------------------------------------------
// Pair28Form: lane pairs on the carry-free bucket state (ec28_lp.h: xyzz28_lp_add), as Quad28Form for G1 -- the buckets come
// as the accumulation kernel keeps them (two XYZZ28L per bucket, one per lane; ZZ = 0 limbs in both for an empty bucket),
// the chunk sums stay in that form, the W x nsel sums that travel to the host leave in the boundary form.  The lane's value,
// its loads, stores and conversion are G2Form28's.  No prefetch in the chunk loop: k_chunks_lp28 sits at 256 VGPRs.
template <class C>
__device__ __noinline__ void xyzz28_lp_add_ool(XYZZ28L<Fp28<C>>& acc, bool& inf, const XYZZ28L<Fp28<C>>& q, bool q_inf) {
  xyzz28_lp_add<C, PairDevice<C>>(acc, inf, q, q_inf);
}
template <class C>
struct Pair28Form {
  typedef G2Form28<C> Fm;
  static constexpr int LANES = 2;
  static constexpr bool CHUNK_PREFETCH = false, TREE_HAND_OVER = true;
  typedef Fp2Field<C> BF;
  typedef XYZZ28L<Fp28<C>> Mem;  // (two per point: MEMS)
  typedef typename Fm::Acc V;
  static __device__ __forceinline__ int hi() { return (int)(threadIdx.x & 1u); }
  static constexpr int MEMS = 2;
  static __device__ __forceinline__ void set_empty(V& v) { Fm::set_identity(v); }
  static __device__ __forceinline__ void load(V& v, const Mem* arr, size_t i) { Fm::load_state(v, arr, i, hi()); }
  static __device__ __forceinline__ void store(Mem* arr, size_t i, const V& v) { Fm::store_state(arr, i, v, hi()); }
  static __device__ __forceinline__ void add(V& a, const V& b) { xyzz28_lp_add_ool<C>(a.p, a.inf, b.p, b.inf); }
  static __device__ __forceinline__ void store_out(XYZZ<BF>* out, size_t i, const V& v) {
    typename Fm::LaneB r;
    Fm::to_boundary(r, v);
    Fm::store_lane(out, i, r, hi());
  }
};

// boundary form (MLHIP_REDUCE32 / MLHIP_ACC32, test build)
template <class C>
__global__ void __launch_bounds__(256) k_chunks_lp(const XYZZ<Fp2Field<C>>* __restrict__ buckets, size_t n_chunks, int l_eff,
                                                   XYZZ<Fp2Field<C>>* __restrict__ A, XYZZ<Fp2Field<C>>* __restrict__ W0) {
  reduce_chunks_body<PairForm<C>>(buckets, n_chunks, l_eff, A, W0);
}
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_masked_sums_lp(const XYZZ<Fp2Field<C>>* __restrict__ A,
                                                          const XYZZ<Fp2Field<C>>* __restrict__ W0, uint32_t T, int nsel,
                                                          XYZZ<Fp2Field<C>>* __restrict__ out) {
  reduce_masked_body<PairForm<C>, BLOCK>(A, W0, T, nsel, out);
}

// carry-free form: the G2 reduction
template <class C>
__global__ void __launch_bounds__(256) k_chunks_lp28(const XYZZ28L<Fp28<C>>* __restrict__ buckets, size_t n_chunks, int l_eff,
                                                     XYZZ28L<Fp28<C>>* __restrict__ A, XYZZ28L<Fp28<C>>* __restrict__ W0) {
  reduce_chunks_body<Pair28Form<C>>(buckets, n_chunks, l_eff, A, W0);
}
// Written out, not over reduce_masked_body: with the lane's value as Pair28Form::V (state and flag in one struct, handed to
// the out-of-line addition by reference) the kernel needed 16 B more scratch per lane on the 14-limb curves than with the
// loose states and flags below.  Same lists (reduce_sel_index), same tree schedule (the upper half of the pairs hands its
// sums to the lower half, then PAIRS / 2 slots of two lane entries), same exit as Pair28Form::store_out.
template <class C>
__device__ __forceinline__ bool lp28_load_state(XYZZ28L<Fp28<C>>& r, const XYZZ28L<Fp28<C>>* src, size_t idx, int hi) {
  r = src[2 * idx + hi];
  return lp28_all_zero<C, PairDevice<C>>(r.zz);  // infinity
}
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_masked_sums_lp28(const XYZZ28L<Fp28<C>>* __restrict__ A,
                                                            const XYZZ28L<Fp28<C>>* __restrict__ W0, uint32_t T, int nsel,
                                                            XYZZ<Fp2Field<C>>* __restrict__ out) {
  typedef XYZZ28L<Fp28<C>> X;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  X* sh = reinterpret_cast<X*>(smem);
  constexpr uint32_t PAIRS = BLOCK / 2;
  const uint32_t pid = threadIdx.x >> 1;
  const int hi = (int)(threadIdx.x & 1u);
  const uint32_t w = blockIdx.x / nsel;
  const int sel = blockIdx.x % nsel;
  const X* src = (sel < 2 ? W0 : A) + (size_t)2 * w * T;
  X acc, b;
  bool inf = true;
  const uint32_t count = reduce_sel_count(sel, T);
  for (uint32_t j = pid; j < count; j += PAIRS) {
    const bool b_inf = lp28_load_state<C>(b, src, reduce_sel_index(sel, j, T), hi);
    xyzz28_lp_add_ool<C>(acc, inf, b, b_inf);
  }
  if (pid >= PAIRS / 2) lp28_store_state<C>(sh, pid - PAIRS / 2, acc, inf, hi);
  __syncthreads();
  if (pid < PAIRS / 2) {
    const bool b_inf = lp28_load_state<C>(b, sh, pid, hi);
    xyzz28_lp_add_ool<C>(acc, inf, b, b_inf);
  }
  __syncthreads();
  if (pid < PAIRS / 2) lp28_store_state<C>(sh, pid, acc, inf, hi);
  __syncthreads();
  for (uint32_t s = PAIRS / 4; s > 0; s >>= 1) {
    if (pid < s) {  // pair-uniform
      const bool b_inf = lp28_load_state<C>(b, sh, pid + s, hi);
      xyzz28_lp_add_ool<C>(acc, inf, b, b_inf);
      lp28_store_state<C>(sh, pid, acc, inf, hi);
    }
    __syncthreads();
  }
  if (pid == 0) {
    typename G2Form28<C>::Acc r{acc, inf};
    Pair28Form<C>::store_out(out, blockIdx.x, r);
  }
}

// the combine of a folded G2 plan (msm_reduce.h: group_combine_body), in the boundary form; launched with 4 W threads
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_group_combine_lp(const XYZZ<Fp2Field<C>>* __restrict__ in, int W, int nsel, int nb,
                                                            XYZZ<Fp2Field<C>>* __restrict__ out) {
  group_combine_body<PairForm<C>>(in, W, nsel, nb, out);
}

}  // namespace mlhip
