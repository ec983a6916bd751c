// msm_reduce.h -- bucket reduction: the three levels (chunk sums, the W x nsel half / bit-masked sums, the group combine of
// folded plans) and the LDS tree over a workgroup's lane groups, each written once over a reduction form ("reduction
// forms" below), with the G1 forms (one lane, quads in the boundary form, quads in the carry-free form) and their kernels.
// The two G2 forms and their kernels are in msm_g2.h.  Part of msm_kernels.h.
#pragma once
// (included by msm_kernels.h after its common headers and constants)

namespace mlhip {

// out-of-line group operations for kernels that use several of them (bounds the code size)
template <class F>
__device__ __noinline__ void xyzz_madd_ool(XYZZ<F>& acc, const Affine<F>& q) {
  xyzz_madd<F>(acc, q, false);
}
template <class F>
__device__ __noinline__ void xyzz_add_ool(XYZZ<F>& acc, const XYZZ<F>& q) {
  xyzz_add<F>(acc, q);
}
template <class F>
__device__ __noinline__ void xyzz_dbl_ool(XYZZ<F>& r, const XYZZ<F>& p) {
  xyzz_dbl<F>(r, p);
}

// one XYZZ per quad of lanes (ec_quad.h): lane q of a quad holds coordinate q (X, Y, ZZ, ZZZ)
template <class C>
__device__ __forceinline__ void quad_load(Fp<C>& v, const XYZZ<FpField<C>>* arr, size_t idx) {
  v = reinterpret_cast<const Fp<C>*>(arr + idx)[threadIdx.x & 3u];
}
template <class C>
__device__ __forceinline__ void quad_store(XYZZ<FpField<C>>* arr, size_t idx, const Fp<C>& v) {
  reinterpret_cast<Fp<C>*>(arr + idx)[threadIdx.x & 3u] = v;
}
template <class C>
__device__ __forceinline__ void quad_set_inf(Fp<C>& v) {  // (1, 1, 0, 0)
  Fp<C> one, zero;
  fp_one<C>(one);
  fp_zero<C>(zero);
  fp_select<C>(v, (threadIdx.x & 2u) != 0, zero, one);
}
// ... and one carry-free XYZZ28 per quad (ec_quad28.h)
template <class C>
__device__ __forceinline__ void quad28_load(Fp28<C>& v, const XYZZ28<C>* arr, size_t idx) {
  v = reinterpret_cast<const Fp28<C>*>(arr + idx)[threadIdx.x & 3u];
}
template <class C>
__device__ __forceinline__ void quad28_store(XYZZ28<C>* arr, size_t idx, const Fp28<C>& v) {
  reinterpret_cast<Fp28<C>*>(arr + idx)[threadIdx.x & 3u] = v;
}

// ---- reduction forms ------------------------------------------------------------------------------------------------
// The levels below are written once over a form R, which is the only place that knows how one point is spread over LANES
// adjacent lanes (a lane group; every branch of the bodies is group-uniform) and how two such points are added.  A form
// supplies, per lane:
//   LANES             1, 2 or 4
//   Mem, MEMS         the element type of buckets / A / W0 and of the LDS slots, and how many of them make a point
//   BF                the boundary field of `out`
//   V, set_empty      the lane's value (with its infinity flag where the form has one) and the empty sum
//   load, store, add  point i of an array into / from the lane's value; the group addition
//   store_out         the lane's part of the boundary-form XYZZ<BF> that leaves through d_out
// and the schedule its kernels were measured with:
//   CHUNK_PREFETCH    the chunk loop loads the next bucket under the additions of this one (msm_body.h: reduce_chunk_body)
//   TREE_HAND_OVER    the tree of the masked sums starts by handing the upper half of the groups' sums to the lower half,
//                     so it needs half the slots (group_tree_sum)
// Forms: LaneForm (one lane, boundary form; test build), QuadForm (quads, boundary form: the test build's reduction, the
// combine of folded plans and the tree of the long buckets), Quad28Form (quads on the accumulation's own carry-free state,
// Weierstrass or Edwards: the G1 reduction); PairForm and Pair28Form (msm_g2.h) are the same for G2 on lane pairs.
template <class F>
struct LaneForm : ChunkLaneForm<F> {  // (msm_body.h: Mem, V, set_empty, load, store)
  static constexpr int LANES = 1;
  static constexpr bool TREE_HAND_OVER = false;
  typedef F BF;
  typedef XYZZ<F> V;
  static __device__ __forceinline__ void add(V& a, const V& b) { xyzz_add_ool<F>(a, b); }
  static __device__ __forceinline__ void store_out(XYZZ<BF>* out, size_t i, const V& v) { out[i] = v; }
};

// one point per QUAD of lanes (ec_quad.h): a group addition is 4 rounds of one field product per lane instead of 14 in a row
template <class C>
struct QuadForm {
  static constexpr int LANES = 4;
  static constexpr bool CHUNK_PREFETCH = true, TREE_HAND_OVER = false;
  typedef FpField<C> BF;
  typedef XYZZ<BF> Mem;
  typedef Fp<C> V;
  static constexpr int MEMS = 1;
  static __device__ __forceinline__ void set_empty(V& v) { quad_set_inf<C>(v); }
  static __device__ __forceinline__ void load(V& v, const Mem* arr, size_t i) { quad_load<C>(v, arr, i); }
  static __device__ __forceinline__ void store(Mem* arr, size_t i, const V& v) { quad_store<C>(arr, i, v); }
  static __device__ __forceinline__ void add(V& a, const V& b) { quad_xyzz_add<C, QuadDevice<C>>(a, b); }
  static __device__ __forceinline__ void store_out(XYZZ<BF>* out, size_t i, const V& v) { quad_store<C>(out, i, v); }
};

// The quad-lane reduction on the accumulation kernels' own bucket state (XYZZ28, ec_quad28.h): buckets come as the carry-free
// accumulators (ZZ all-zero limbs = empty), the chunk sums stay in that form, and only the W x nsel sums that travel to the
// host are converted to the boundary form (one conversion per lane).  ED: the buckets arrive in extended twisted Edwards
// coordinates (a subgroup-trusted BLS12-377 plan, msm_ed.h); the empty sum is the identity (0 : 1 : 1 : 0) and the addition
// ed_quad28_add: three product rounds instead of four, no exceptional case.
template <class C, bool ED>
struct Quad28Form {
  static constexpr int LANES = 4;
  static constexpr bool CHUNK_PREFETCH = true, TREE_HAND_OVER = false;
  typedef FpField<C> BF;
  typedef XYZZ28<C> Mem;
  typedef Fp28<C> V;
  static constexpr int MEMS = 1;
  static __device__ __forceinline__ void set_empty(V& v) {
    fp28_zero<C>(v);
    if constexpr (ED) {
      Fp28<C> one;
      fp28_from_const<C>(one, C::ONE28);
      const unsigned q = threadIdx.x & 3u;
      fp28_select<C>(v, q == 1 || q == 2, one, v);
    }
  }
  static __device__ __forceinline__ void load(V& v, const Mem* arr, size_t i) { quad28_load<C>(v, arr, i); }
  static __device__ __forceinline__ void store(Mem* arr, size_t i, const V& v) { quad28_store<C>(arr, i, v); }
  static __device__ __forceinline__ void add(V& a, const V& b) {
    if constexpr (ED)
      ed_quad28_add<C, QuadDevice28<C>>(a, b);
    else
      quad28_xyzz_add<C, QuadDevice28<C>>(a, b);
  }
  static __device__ __forceinline__ void store_out(XYZZ<BF>* out, size_t i, const V& v) {
    Fp<C> r;
    if constexpr (ED) {
      // the W x nsel sums leave as Weierstrass points in the boundary form, like every other path's: each lane of the
      // quad rebuilds the point from the four coordinates and keeps its own
      XYZZ28<C> g4, w;
      QuadDevice28<C>::gather(g4, v);
      EdExt28<C> e;
      e.x = g4.x;
      e.y = g4.y;
      e.z = g4.zz;
      e.t = g4.zzz;
      bool inf;
      ed28_to_xyzz28<C>(w, inf, e);
      XYZZ<FpField<C>> r4;
      xyzz28_to<C>(r4, w, inf);
      const unsigned q = threadIdx.x & 3u;
      Fp<C> t2;
      fp_select<C>(t2, q == 0, r4.x, r4.y);
      fp_select<C>(r, q >= 2, r4.zz, t2);
      fp_select<C>(r, q == 3, r4.zzz, r);
    } else {
      fp28_to_fp<C>(r, v);  // (an empty sum is ZZ = 0 limbs, which converts to the boundary form's ZZ = 0)
    }
    quad_store<C>(out, i, r);
  }
};

// ---- the LDS tree --------------------------------------------------------------------------------------------------
// Sum over the first n lane groups of a workgroup (n a power of two; group gid brings `acc`, all threads must call): on
// return group 0 holds the sum in acc and in slot 0 of sh.  HAND_OVER: the upper half of the groups hands its sums to the
// lower half first, so that n / 2 slots are enough (the G2 masked sums: 48 / 56 KB for 512 threads -- twice the pairs per
// block, half the strided additions per pair, one more tree level).
template <class R, bool HAND_OVER = false>
__device__ __forceinline__ void group_tree_sum(typename R::Mem* sh, typename R::V& acc, uint32_t gid, uint32_t n) {
  if constexpr (HAND_OVER) {
    n >>= 1;
    if (gid >= n) R::store(sh, gid - n, acc);
    __syncthreads();
    if (gid < n) {
      typename R::V v;
      R::load(v, sh, gid);
      R::add(acc, v);
    }
    __syncthreads();
    if (gid < n) R::store(sh, gid, acc);
  } else {
    R::store(sh, gid, acc);
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = n / 2; s > 0; s >>= 1) {
    if (gid < s) {  // group-uniform
      typename R::V v;
      R::load(v, sh, gid + s);
      R::add(acc, v);
      R::store(sh, gid, acc);
    }
    __syncthreads();
  }
}

// LDS tree sum of one XYZZ per thread; result valid in sh[0] after return (all threads must call)
template <class F, int BLOCK>
__device__ void block_tree_sum(XYZZ<F>* sh, const XYZZ<F>& mine) {
  const int tid = threadIdx.x;
  sh[tid] = mine;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
      XYZZ<F> a = sh[tid];
      xyzz_add_ool<F>(a, sh[tid + s]);
      sh[tid] = a;
    }
    __syncthreads();
  }
}

// The same for G1 with one point per QUAD of lanes: a group addition is 4 rounds of one field product per lane instead of 14
// in a row, so the 8 dependent levels cost ~3x less (the tree is pure latency: one workgroup, one slice).  BLOCK / 4 quads
// first fold four entries each, then halve.  Written out, not over group_tree_sum: on the shared tree the long-bucket kernels
// that call it left the figures of the hand-written one (k_big_slices<FpField<Bn254>, 256> one VGPR more, SGPR spills of
// k_accumulate_big_seg<Bls377 / Bls381> and k_accumulate_big_seg_ed up by 3, 15 and 12).
template <class C, int BLOCK>
__device__ void block_tree_sum_q(XYZZ<FpField<C>>* sh, const XYZZ<FpField<C>>& mine) {
  typedef QuadDevice<C> B;
  constexpr uint32_t NQ = BLOCK / 4;
  const uint32_t quad = threadIdx.x >> 2;
  sh[threadIdx.x] = mine;
  __syncthreads();
  Fp<C> acc, v;
  quad_load<C>(acc, sh, quad);
#pragma unroll 1
  for (uint32_t j = 1; j < 4; j++) {
    quad_load<C>(v, sh, quad + j * NQ);
    quad_xyzz_add<C, B>(acc, v);
  }
  __syncthreads();  // every entry has been read
  quad_store<C>(sh, quad, acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = NQ / 2; s > 0; s >>= 1) {
    if (quad < s) {  // quad-uniform
      quad_load<C>(v, sh, quad + s);
      quad_xyzz_add<C, B>(acc, v);
      quad_store<C>(sh, quad, acc);
    }
    __syncthreads();
  }
}

// the tree the long-bucket kernels use: quads for G1, one lane per point for G2
template <class F, int BLOCK>
__device__ __forceinline__ void block_tree_sum_auto(XYZZ<F>* sh, const XYZZ<F>& mine) {
  if constexpr (std::is_same<F, FpField<typename F::Curve>>::value)
    block_tree_sum_q<typename F::Curve, BLOCK>(sh, mine);
  else
    block_tree_sum<F, BLOCK>(sh, mine);
}

// ---- the three levels ----------------------------------------------------------------------------------------------
// Level 1: lane group g owns the l_eff buckets of chunk g (msm_body.h: reduce_chunk_body).
template <class R>
struct FormAdd {
  __device__ __forceinline__ void operator()(typename R::V& a, const typename R::V& b) const { R::add(a, b); }
};
template <class R>
__device__ __forceinline__ void reduce_chunks_body(const typename R::Mem* __restrict__ buckets, size_t n_chunks, int l_eff,
                                                   typename R::Mem* __restrict__ A, typename R::Mem* __restrict__ W0) {
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / R::LANES;
  if (g >= n_chunks) return;  // group-uniform
  reduce_chunk_body<R>(g, buckets, A, W0, l_eff, FormAdd<R>());
}

// Level 2: block (w, sel) sums list sel of window w (msm_body.h: reduce_sel_index) -- BLOCK / LANES groups stride over the
// list, then the tree; the sum leaves in the boundary form.
template <class R, int BLOCK>
__device__ __forceinline__ void reduce_masked_body(const typename R::Mem* __restrict__ A, const typename R::Mem* __restrict__ W0,
                                                   uint32_t T, int nsel, XYZZ<typename R::BF>* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typename R::Mem* sh = reinterpret_cast<typename R::Mem*>(smem);
  constexpr uint32_t GROUPS = BLOCK / R::LANES;
  const uint32_t gid = threadIdx.x / R::LANES;
  const uint32_t w = blockIdx.x / nsel;
  const int sel = blockIdx.x % nsel;
  const typename R::Mem* src = (sel < 2 ? W0 : A) + (size_t)R::MEMS * w * T;
  typename R::V acc;
  R::set_empty(acc);
  const uint32_t count = reduce_sel_count(sel, T);
#pragma unroll 1
  for (uint32_t j = gid; j < count; j += GROUPS) {
    typename R::V v;  // (a value of its own per scope: the lane-pair forms keep it in scratch, and scopes that do not overlap share the slot)
    R::load(v, src, reduce_sel_index(sel, j, T));
    R::add(acc, v);
  }
  group_tree_sum<R, R::TREE_HAND_OVER>(sh, acc, gid, GROUPS);
  if (gid == 0) R::store_out(out, blockIdx.x, acc);
}

// Folded plans (msm_fold.h): the W bucket groups' sums combined on the device.
// Level 2 leaves nsel sums per bucket group g (two halves of sum_t W0[g][t], two halves of sum_t A[g][t], nb bit-masked sums
// of A[g][.]).  For a folded plan the groups are consecutive ranges of ONE bucket set: with the global chunk index
// t' = g T + t the whole MSM is a single "window" of W T chunks,
//   total = sum W0 + sum A + L sum_k 2^k B_k,   B_k = sum of the A[t'] with bit k of t' set, k < nb + lg W,
// and every one of its 2 + nb + lg W sums is a sum of at most 2 W entries of `in`: B_k = sum_g in[g][4 + k] for k < nb, and
// the plain sums in[g][2] + in[g][3] of the groups g with bit k - nb set above.  One block per output, one lane group per
// input slot (group g = gid / 2, half h = gid & 1; fold_combine_src), then the tree over the 2 W slots; the host tail is
// then that of ONE window (nb + lg W + lg L doublings, no per-group work on the host pool): 0.083 -> 0.04 ms at c = 20 for
// G1, 0.30 ms -> one window's 19 doublings on the calling thread for a 2^20-point G2 MSM.
// out = [sum W0 | sum A | inf | inf | B_0 .. B_(nb + lgW - 1)]: the layout host_tail_window reads.  W a power of two <= 32.
template <class R>
__device__ __forceinline__ void group_combine_body(const XYZZ<typename R::BF>* __restrict__ in, int W, int nsel, int nb,
                                                   XYZZ<typename R::BF>* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typename R::Mem* sh = reinterpret_cast<typename R::Mem*>(smem);
  const uint32_t gid = threadIdx.x / R::LANES;
  const int o = blockIdx.x;  // output index in the layout above
  const uint32_t n = 2u * (uint32_t)W;
  typename R::V acc;
  R::set_empty(acc);
  if (gid < n) {  // group-uniform
    const int g = (int)(gid >> 1);
    const int src = fold_combine_src(o, g, (int)(gid & 1u), nb);
    if (src >= 0) R::load(acc, in, (size_t)g * nsel + src);
  }
  group_tree_sum<R>(sh, acc, gid, n);
  if (gid == 0) R::store(out, (size_t)o, acc);
}

// ---- the G1 kernels ------------------------------------------------------------------------------------------------
// one lane per point, boundary form (MLHIP_REDUCE_ONE_LANE, test build)
template <class F>
__global__ void __launch_bounds__(256) k_chunks(const XYZZ<F>* __restrict__ buckets, size_t n_chunks, int l_eff,
                                                XYZZ<F>* __restrict__ A, XYZZ<F>* __restrict__ W0) {
  reduce_chunks_body<LaneForm<F>>(buckets, n_chunks, l_eff, A, W0);
}
template <class F, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_masked_sums(const XYZZ<F>* __restrict__ A, const XYZZ<F>* __restrict__ W0,
                                                       uint32_t T, int nsel, XYZZ<F>* __restrict__ out) {
  reduce_masked_body<LaneForm<F>, BLOCK>(A, W0, T, nsel, out);
}

// one point per quad, boundary form (MLHIP_REDUCE32, test build)
template <class C>
__global__ void __launch_bounds__(256) k_chunks_q(const XYZZ<FpField<C>>* __restrict__ buckets, size_t n_chunks, int l_eff,
                                                  XYZZ<FpField<C>>* __restrict__ A, XYZZ<FpField<C>>* __restrict__ W0) {
  reduce_chunks_body<QuadForm<C>>(buckets, n_chunks, l_eff, A, W0);
}
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_masked_sums_q(const XYZZ<FpField<C>>* __restrict__ A,
                                                         const XYZZ<FpField<C>>* __restrict__ W0, uint32_t T, int nsel,
                                                         XYZZ<FpField<C>>* __restrict__ out) {
  reduce_masked_body<QuadForm<C>, BLOCK>(A, W0, T, nsel, out);
}

// one point per quad on the carry-free bucket state: the G1 reduction.  (The two additions of a bucket are written out in
// the chunk loop since round 4: one loop body that selected its operands cost 56 selects per step, reduction 0.420 ->
// 0.410 ms at 2^20, profiles/r04_chunks_two_ab.txt.)
template <class C, bool ED = false>
__global__ void __launch_bounds__(256) k_chunks_q28(const XYZZ28<C>* __restrict__ buckets, size_t n_chunks, int l_eff,
                                                    XYZZ28<C>* __restrict__ A, XYZZ28<C>* __restrict__ W0) {
  reduce_chunks_body<Quad28Form<C, ED>>(buckets, n_chunks, l_eff, A, W0);
}
template <class C, int BLOCK, bool ED = false>
__global__ void __launch_bounds__(BLOCK) k_masked_sums_q28(const XYZZ28<C>* __restrict__ A, const XYZZ28<C>* __restrict__ W0,
                                                           uint32_t T, int nsel, XYZZ<FpField<C>>* __restrict__ out) {
  reduce_masked_body<Quad28Form<C, ED>, BLOCK>(A, W0, T, nsel, out);
}

// the combine of a folded G1 plan, in the boundary form (both carry-free forms leave Weierstrass sums); launched with
// max(64, 8 W) threads
template <class C, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_group_combine_q(const XYZZ<FpField<C>>* __restrict__ in, int W, int nsel, int nb,
                                                           XYZZ<FpField<C>>* __restrict__ out) {
  group_combine_body<QuadForm<C>>(in, W, nsel, nb, out);
}

}  // namespace mlhip
