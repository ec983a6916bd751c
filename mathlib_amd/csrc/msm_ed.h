// msm_ed.h -- G1 bucket accumulation in extended twisted Edwards coordinates (ed28.h) for plans whose caller vouches for
// the prime-order subgroup (mlhip_msm_plan_assume_srs; curves with C::HAS_EDWARDS: BLS12-377).  Part of msm_kernels.h.
// EdForm28 is the bucket form; its kernels are the shared bodies of msm_accumulate.h on it: same entry lists, same state
// buffer (an EdExt28 has the footprint of an XYZZ28).  The buckets STAY in extended Edwards coordinates: the quad-lane
// reduction kernels run their Edwards instantiation on them (msm_reduce.h: Quad28Form<C, true>, ed_quad28_add) and
// only the W x nsel window sums return to the Weierstrass curve, for the host tail.
#pragma once
// (included by msm_kernels.h after msm_accumulate.h)

namespace mlhip {

// Weierstrass affine (boundary form) -> halved Niels triples, four points per thread sharing one inversion
template <class C>
__global__ void __launch_bounds__(256) k_points_to_ed28(const Affine<FpField<C>>* __restrict__ points, size_t n,
                                                        EdNiels28<C>* __restrict__ out) {
  constexpr int K = 4;
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * K;
  if (i0 >= n) return;
  Affine<FpField<C>> in[K];
  Fp<C> xh[K], yh[K];
#pragma unroll
  for (int j = 0; j < K; j++) {
    if (i0 + j < n) {
      in[j] = points[i0 + j];
    } else {  // padding: the point at infinity
      fp_zero<C>(in[j].x);
      fp_zero<C>(in[j].y);
    }
  }
  ed_affine_halves_batch<C, K>(xh, yh, in);
#pragma unroll
  for (int j = 0; j < K; j++) {
    if (i0 + j < n) {
      EdNiels28<C> q;
      ed_niels_from_halves<C>(q, xh[j], yh[j]);
      out[i0 + j] = q;
    }
  }
}

// The Edwards bucket form (see "bucket forms", msm_accumulate.h): Niels rows, EdExt28 accumulators and state -- the identity
// is a value, there is no infinity flag -- in the buffer the Weierstrass form keeps its XYZZ28 in.  The buckets never take
// the boundary form; what it inherits from G1Form28 is the boundary form of the slice sums, which the combine reads.
template <class C>
struct EdForm28 : G1Form28<C> {
  static_assert(sizeof(EdExt28<C>) == sizeof(XYZZ28<C>), "the two bucket forms share the state buffer");
  static constexpr bool HAS_BOUNDARY = false;
  typedef FpField<C> BF;
  typedef EdNiels28<C> RowMem, Row;
  typedef XYZZ28<C> State;
  typedef XYZZ<BF> LaneB;
  typedef EdExt28<C> Acc;
  static __device__ __forceinline__ void load_row(Row& r, const RowMem* rows, uint32_t i, int) { r = rows[i]; }
  MLHIP_HD static void set_identity(Acc& a) { ed28_set_identity<C>(a); }
  MLHIP_HD static void madd(Acc& a, const Row& q, bool negate) { ed28_madd<C>(a, q, negate); }
  static __device__ __forceinline__ void load_state(Acc& a, const State* state, size_t g, int) {
    a = reinterpret_cast<const EdExt28<C>*>(state)[g];
  }
  static __device__ __forceinline__ void store_state(State* state, size_t g, const Acc& a, int) {
    reinterpret_cast<EdExt28<C>*>(state)[g] = a;
  }
  MLHIP_HD static void to_boundary(LaneB& r, const Acc& a) {
    XYZZ28<C> w;
    bool inf;
    ed28_to_xyzz28<C>(w, inf, a);
    xyzz28_to<C>(r, w, inf);
  }
  // the combine adds the bucket's earlier state on the Weierstrass side and maps the total back to extended Edwards
  // coordinates (two inversions; a handful of buckets per segment)
  static __device__ __forceinline__ bool state_to_boundary(XYZZ<BF>& r, const State* state, size_t g) {
    Acc e;
    load_state(e, state, g, 0);
    to_boundary(r, e);
    return true;
  }
  static __device__ __forceinline__ void boundary_to_state(State* state, size_t g, const XYZZ<BF>& sum) {
    Affine<BF> a;
    xyzz_to_affine<BF>(a, sum);  // (0, 0) for the point at infinity: ed28_from_affine maps it to the identity
    Acc e;
    ed28_from_affine<C>(e, a);
    store_state(state, g, e, 0);
  }
};

// state[g] is the bucket in extended coordinates, between segments and for the reduction
template <class C>
__global__ void __launch_bounds__(256) k_accumulate_ed28_seg(const EdNiels28<C>* __restrict__ points,
                                                             const uint32_t* __restrict__ sorted,
                                                             const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ counts, size_t n_buckets,
                                                             const uint32_t* __restrict__ order, uint32_t big_threshold,
                                                             uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
                                                             XYZZ28<C>* __restrict__ state, int flags) {
  accumulate_seg_body<EdForm28<C>>(points, sorted, offsets, counts, n_buckets, order, big_threshold, big_list, big_count, state,
                                   flags, nullptr);
}

// (the slice sums come in the boundary form: from k_big_slices on the original points, or k_big_slices28 on the Niels rows)
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_accumulate_big_seg_ed(const uint32_t* __restrict__ big_list,
                                                                 const uint32_t* __restrict__ big_count,
                                                                 const uint32_t* __restrict__ prefix,
                                                                 const XYZZ<FpField<C>>* __restrict__ partials,
                                                                 XYZZ28<C>* __restrict__ state, int flags) {
  accumulate_big_body<EdForm28<C>, BLOCK>(big_list, big_count, prefix, partials, state, flags, nullptr);
}

// the slice sums of long G1 buckets from the carry-free rows: Weierstrass rows or, ED, Niels triples
template <class C, int BLOCK, bool ED>
__global__ void __launch_bounds__(BLOCK) k_big_slices28(const void* __restrict__ rows, const uint32_t* __restrict__ sorted,
                                                        const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ big_list, const uint32_t* __restrict__ big_count,
                                                        const uint32_t* __restrict__ prefix,
                                                        XYZZ<FpField<C>>* __restrict__ partials) {
  typedef typename std::conditional<ED, EdForm28<C>, G1Form28<C>>::type Fm;
  big_slices_body<Fm, BLOCK>(static_cast<const typename Fm::RowMem*>(rows), sorted, offsets, counts, big_list, big_count, prefix,
                             partials);
}
}  // namespace mlhip
