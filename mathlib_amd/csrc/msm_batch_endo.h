// msm_batch_endo.h -- the Straus chunks of mlhip_msm_batch* for points the caller PROMISES to be in G1 / G2 (the prime-order
// subgroup, or the point at infinity): MLHIP_CURVE_SUBGROUP_POINTS(curve_id) of include/mlhip.h, DESIGN.md section 19.
// Part of msm_kernels.h (after msm_batch.h and msm_scalar_mul_endo.h); the two per-lane bodies are plain __host__ __device__,
// so tests/hostmath_batch_endo replays them on the CPU.
//
// The chunk of msm_batch.h (a table per pair, doublings shared by the chunk's P pairs) over the scalar splits of
// msm_scalar_mul_endo.h (short scalars per pair, so fewer doublings to share).  Group operations per pair:
//     plain chunk                                                        256 / P + 7 + <= 65
//     G1, BLS12   s = a + b x^2, a, b < 2^128: 33 joint signed 4-bit windows, ONE table {1 .. 8}P_j per pair; an addition
//                 for b reads the same entry, scales X by beta and flips Y    128 / P + 7 + <= 66
//     G2, BLS12   four digits base |x| over Q, psi Q, psi^2 Q, psi^3 Q: the 15-entry subset table per pair, 64 steps of
//                 one doubling and at most one addition per pair               64 / P + 11 + <= 64
//     G2, BN254   two digits base 6 x^2, table [a]Q + [b]psi Q (a, b <= 3), 64 steps of two doublings
//                                                                            128 / P + 13 + <= 64
//     G1, BN254   s = k1 + k2 lambda, |k1|, |k2| < 2^127 (g1_glv_split; G1Glv<C>, not ScalarMulEndo<C, true>): the G1 body
//                 of the BLS12 curves with the signs of k1, k2 per pair            128 / P + 7 + <= 66
// The G2 table is 15 XYZZ per pair where the plain chunk's is 8, all of it scratch: the split chunks are compiled for
// P = 1, 2, 4 on G2 (P = 4 on a BLS12 curve: 11.5 KB per lane), and at MLHIP_MSM_BATCH_CHUNK=8 a promised G2 call runs the
// plain chunk kernel.
// A point outside the subgroup gives a wrong partial for its own chunk -- its own segment -- and nothing else: every address
// and every branch depends on the scalars alone, every operation is the complete XYZZ arithmetic of the plain chunk.
// Measured (profiles/msm_batch_endo_ab.txt; flagged / plain time at the same P over 2^10 .. 2^16 segments
// of 2 .. 64 pairs, counted ratio in brackets): G1 0.68 - 0.77 at P = 1 (0.61), 0.78 - 0.90 at P = 4 (0.78), 0.81 - 0.97 at P = 8
// (0.86); G2 of the BLS12 curves 0.51 - 0.62 at P = 1 (0.43), 0.64 - 0.86 at P = 4 (0.67); G2 of BN254 0.71 - 0.80 at P = 1 (0.63),
// 0.79 - 0.97 at P = 4 (0.81).  Above the counts because only doublings go, the cheapest operation.  Ahead of the plain call
// in every cell at the default P = 4, which flagged calls keep: all five (curve, group) with a split take it by default.
// G1 of BN254 (profiles/msm_batch_glv_ab.txt): 0.67 - 0.80 at P = 1 (0.61), 0.76 - 0.88 at P = 4 (0.78),
// 0.76 - 0.92 at P = 8 (0.86), ahead in every cell at P = 4 as well: the sixth takes it too.
// Layout, sum passes, scratch buffer, event ordering and the bucket route of the long segments are those of msm_batch.h /
// msm_batch_bucket.h, unchanged: a promised call differs in the chunk kernel alone.
#pragma once
#include "msm_batch.h"
#include "msm_scalar_mul_endo.h"

namespace mlhip {

// the chunk lengths the split chunks are compiled for (G2: the table of P = 8 would be 23 KB of scratch per lane)
template <bool G1>
constexpr bool msm_batch_endo_p_compiled(int p) {
  return p == 1 || p == 2 || p == 4 || (G1 && p == 8);
}

// acc = sum_{j < count} [s_j] P_j for one chunk (count <= P) of points in G1; scalars, load as in
// msm_batch_chunk.  Per pair the windows of a and b (five words each: both are below 2^128, so window 32 holds the carry
// and nothing lies above) and the table {1 .. 8}P_j; then windows 32 .. 0, a's digit on the table entry and b's digit on the
// same entry with X beta and Y flipped (BN254: flipped as the signs of k1, k2 say) -- g1_endo_chain for P pairs at once.
template <class F, int P, class Ops, class Load>
MLHIP_HD void msm_batch_chunk_endo_g1(XYZZ<F>& acc, const uint32_t* scalars, uint32_t count, bool mont, Load load) {
  typedef typename F::Curve C;
  typedef G1Split<C> S;
  uint32_t wa[P][5], wb[P][5];
  uint32_t negs = 0;  // BN254: bit 2 j + half = the sign of pair j's k1 / k2 (BLS12: constants, this word is never read)
  XYZZ<F> tab[P][8];
#pragma unroll 1
  for (int j = 0; j < P; j++) {
    uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a[8], b[8], t[9];
    if ((uint32_t)j < count) fr_canonical<C>(s, scalars + 8 * j, mont);
    bool neg_a, neg_b;
    S::split(a, b, neg_a, neg_b, s);  // s = 0 (a slot past the chunk's end): a = b = 0, every digit 0, the table is never read
    if (!S::FIXED_SIGNS) negs |= ((neg_a ? 1u : 0u) | (neg_b ? 2u : 0u)) << (2 * j);
    signed_windows4(t, a);
#pragma unroll
    for (int k = 0; k < 5; k++) wa[j][k] = t[k];
    signed_windows4(t, b);
#pragma unroll
    for (int k = 0; k < 5; k++) wb[j][k] = t[k];
    if ((uint32_t)j >= count) continue;
    Affine<F> pt;
    load(pt, j);
    xyzz_from_affine<F>(tab[j][0], pt);
#pragma unroll 1
    for (int m = 1; m < 8; m++) {
      tab[j][m] = tab[j][m - 1];
      Ops::madd(tab[j][m], pt);
    }
  }
  typename F::T beta;
  S::beta(beta);
  xyzz_set_inf<F>(acc);
  bool started = false;
#pragma unroll 1
  for (int w = 32; w >= 0; w--) {
    if (started) {
#pragma unroll 1
      for (int d = 0; d < 4; d++) {
        XYZZ<F> t;
        Ops::dbl(t, acc);
        acc = t;
      }
    }
#pragma unroll 1
    for (int jh = 0; jh < 2 * P; jh++) {  // per pair a's digit on +-P_j, then b's digit on (beta x, +-y)
      const int j = jh >> 1, half = jh & 1;
      const int d = signed_window4_digit(half ? wb[j] : wa[j], w);
      if (d) {
        XYZZ<F> q = tab[j][(d < 0 ? -d : d) - 1];
        typename F::T ny;
        F::neg(ny, q.y);
        const bool neg_half = S::FIXED_SIGNS ? half != 0 : ((negs >> jh) & 1u) != 0;
        F::select(q.y, (d < 0) != neg_half, ny, q.y);
        if (half) F::mul(q.x, q.x, beta);
        Ops::add(acc, q);
        started = true;
      }
    }
  }
}

// the same for points in G2: per pair the digits of gt_exp_split and the table of g2_endo_table; then steps 63 .. 0, DBL
// shared doublings and per pair at most one addition of the entry gt_exp_step_index names
template <class F, int P, class Ops, class Load>
MLHIP_HD void msm_batch_chunk_endo_g2(XYZZ<F>& acc, const uint32_t* scalars, uint32_t count, bool mont, Load load) {
  typedef typename F::Curve C;
  uint32_t dig[P][8];
  XYZZ<F> tab[P][15];
#pragma unroll 1
  for (int j = 0; j < P; j++) {
    if ((uint32_t)j >= count) {  // a slot past the chunk's end: every digit 0, the table is never read
#pragma unroll
      for (int k = 0; k < 8; k++) dig[j][k] = 0;
      continue;
    }
    uint32_t s[8];
    fr_canonical<C>(s, scalars + 8 * j, mont);
    gt_exp_split<C>(dig[j], s);
    Affine<F> pt;
    load(pt, j);
    g2_endo_table<C, F, Ops>(tab[j], pt);
  }
  constexpr int DBL = C::IS_BN ? 2 : 1;
  xyzz_set_inf<F>(acc);
  bool started = false;
#pragma unroll 1
  for (int step = 63; step >= 0; step--) {
    if (started) {
#pragma unroll 1
      for (int d = 0; d < DBL; d++) {
        XYZZ<F> t;
        Ops::dbl(t, acc);
        acc = t;
      }
    }
#pragma unroll 1
    for (int j = 0; j < P; j++) {
      const uint32_t m = gt_exp_step_index<C>(dig[j], step);
      if (m) {
        Ops::add(acc, tab[j][m - 1]);
        started = true;
      }
    }
  }
}

#if defined(__HIPCC__)
// ---- kernels: the loads, stores, early-out and launch shapes of k_msm_batch_chunk / k_msm_batch_chunk_lp ------------------
// The group operations are those of EndoOpsG1 / EndoOpsG2Lp (msm_scalar_mul_endo.h) under names of their own: the compiler
// shares ONE out-of-line copy of a policy's large members among the kernels that use it (as it does with MsmBatchOpsG1::add
// and MsmBatchOpsLp::dbl over the four P of the plain chunks), and k_scalar_mul_endo / _lp, each the only user of its policy,
// keep theirs inline -- their code is what it was.  One shared G1 addition (116 KB of code on a BLS12 curve) and one shared
// lane-pair doubling serve the chunk kernels of every P; registers and scratch are the plain chunk kernels' (248 VGPRs on
// the BLS12 curves, the tables in scratch).
template <class C>
struct MsmBatchEndoOpsG1 {
  typedef FpField<C> F;
  __device__ static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
  __device__ static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  __device__ static void madd(XYZZ<F>& acc, const Affine<F>& q) { xyzz_madd_ool<F>(acc, q); }
};
template <class C>
struct MsmBatchEndoOpsLp {
  typedef Fp2LField<C> F;
  __device__ static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
  __device__ static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add_lp_ool<C>(acc, q); }
};

template <class C, int P>
__global__ void __launch_bounds__(64) k_msm_batch_chunk_endo(const Affine<FpField<C>>* __restrict__ points,
                                                             const uint32_t* __restrict__ scalars, int mont,
                                                             const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                             XYZZ<FpField<C>>* __restrict__ partials) {
  typedef FpField<C> F;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const MsmBatchChunk ch = chunks[c];
  if (ch.count > (uint32_t)P) return;  // a slice of a long segment: the bucket kernels write this row (msm_batch_bucket.h)
  const Affine<F>* pts = points + ch.first;
  XYZZ<F> acc;
  msm_batch_chunk_endo_g1<F, P, MsmBatchEndoOpsG1<C>>(acc, scalars + 8 * ch.first, ch.count, mont != 0,
                                              [&](Affine<F>& p, int j) { p = pts[j]; });
  partials[c] = acc;
}

template <class C, int P>
__global__ void __launch_bounds__(64) k_msm_batch_chunk_endo_lp(const Affine<Fp2Field<C>>* __restrict__ points,
                                                                const uint32_t* __restrict__ scalars, int mont,
                                                                const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                                XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair share the chunk and its scalars
  if (c >= n_chunks) return;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchChunk ch = chunks[c];
  if (ch.count > (uint32_t)P) return;  // a slice of a long segment (both lanes of the pair leave): msm_batch_bucket.h
  XYZZ<FL> acc;
  msm_batch_chunk_endo_g2<FL, P, MsmBatchEndoOpsLp<C>>(acc, scalars + 8 * ch.first, ch.count, mont != 0,
                                                 [&](Affine<FL>& p, int j) { lp_load_affine<C>(p, points, ch.first + j, hi); });
  lp_store_xyzz<C>(partials, c, acc, hi);
}

// MLHIP_MSM_BATCH_ENDO=0: every promised call on the plain chunk kernels (second implementation, A/B)
static inline bool msm_batch_endo_enabled() {
  const char* e = getenv("MLHIP_MSM_BATCH_ENDO");
  return !(e && e[0] == '0');
}

// the chunk kernel of a promised call (msm_batch_launch_chunks_p); false: not for this (curve, group, P), or switched off --
// the caller goes on to the plain chunk kernel
template <class C, class F>
bool msm_batch_endo_launch_chunks(int P, const void* d_points, const void* d_scalars, int mont, const MsmBatchChunk* d_chunks,
                                  uint32_t n_chunks, void* d_partials, hipStream_t st) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  if constexpr (!ScalarMulEndo<C, kG1>::AVAILABLE && !(kG1 && G1Glv<C>::AVAILABLE)) {
    return false;
  } else {
    if (!msm_batch_endo_p_compiled<kG1>(P) || !msm_batch_endo_enabled()) return false;
    const Affine<F>* pts = (const Affine<F>*)d_points;
    const uint32_t* sc = (const uint32_t*)d_scalars;
    XYZZ<F>* part = (XYZZ<F>*)d_partials;
    if constexpr (kG1) {
      const dim3 grid((n_chunks + 63) / 64), block(64);
      switch (P) {
        case 1: k_msm_batch_chunk_endo<C, 1><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
        case 2: k_msm_batch_chunk_endo<C, 2><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
        case 4: k_msm_batch_chunk_endo<C, 4><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
        default: k_msm_batch_chunk_endo<C, 8><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
      }
    } else {
      const dim3 grid((unsigned)((2 * (size_t)n_chunks + 63) / 64)), block(64);
      switch (P) {
        case 1: k_msm_batch_chunk_endo_lp<C, 1><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
        case 2: k_msm_batch_chunk_endo_lp<C, 2><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
        default: k_msm_batch_chunk_endo_lp<C, 4><<<grid, block, 0, st>>>(pts, sc, mont, d_chunks, n_chunks, part); break;
      }
    }
    return true;
  }
}
#endif  // __HIPCC__

}  // namespace mlhip
