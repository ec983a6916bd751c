// msm_scalar_mul_endo.h -- batched single-scalar multiplication for points the caller PROMISES to be in G1 / G2 (the
// prime-order subgroup, or the point at infinity): MLHIP_GROUP_SUBGROUP(group) of include/mlhip.h, DESIGN.md section 17.
// Part of msm_kernels.h; the split and the two chains are host-testable (tests/hostmath_endo).
//
// On the subgroup the curve's cheap endomorphisms are multiplications by known scalars, so [s]P splits into short
// multiplications that share their doublings -- the Gt chain of gt_exp_cyclo.h moved to the groups:
//     G1, BLS12:  phi(x, y) = (beta x, y) = [-x^2]P.  With the digits d0 .. d3 of gt_exp_split (base L = |x|),
//                 a = d0 + d1 L, b = d2 + d3 L (both < 2^128), s = a + b x^2 and [s]P = [a]P + [b]P', P' = -phi(P) =
//                 (beta x, -y).  Joint signed 4-bit windows over a and b: 33 windows, 128 doublings, <= 66 additions
//                 against 256 + 65.  ONE table {1 .. 8}P: an addition for b reads the same entry, scales X by beta
//                 (X / ZZ is the affine x) and flips Y.
//     G2, BLS12:  psi(Q) = [x]Q.  s = d0 + d1 L + d2 L^2 + d3 L^3, g_i = psi^i(Q), negated for odd i when x < 0, a 15-entry
//                 Straus table of the subset sums of g0 .. g3, 64 steps of one doubling and at most one addition.
//     G2, BN254:  psi(Q) = [p]Q = [6 x^2]Q =: [L]Q.  s = d0 + d1 L, table [a]Q + [b]psi(Q) for a, b <= 3, 64 steps of two
//                 doublings and at most one addition.
//     G1, BN254:  s = a + b x^2 does not exist; phi(x, y) = (beta x, y) = [lambda]P, lambda = 36 x^4 - 1, and a lattice
//                 reduction gives s = k1 + k2 lambda with |k1|, |k2| < 2^127 (g1_glv_split): the
//                 chain of the BLS12 curves over (|k1|, |k2|) and their signs.  E(Fp) has prime order, so the promise holds
//                 for every point of the curve; GLV_BETA / GLV_LAMBDA are names of their own (G1Glv), ENDO_BETA stays unused.
// A point outside the subgroup gives a wrong value for its own product and nothing else: every address depends on the
// scalar alone, every operation is the complete XYZZ arithmetic of the plain kernels.
#pragma once
#include "ec.h"
#include "gt_exp_cyclo.h"

namespace mlhip {

// does MLHIP_GROUP_SUBGROUP change the chain of this (curve, group)?  (G1: F = FpField<C>)
template <class C, bool G1>
struct ScalarMulEndo {
  static constexpr bool AVAILABLE = G1 ? !C::IS_BN : true;
};

// a = d0 + d1 L, b = d2 + d3 L as eight zero-extended words each (what signed_windows4 reads), BLS12 curves: L < 2^64 and
// every digit < 2^64, so both are below 2^128
MLHIP_HD void endo_mac64(uint32_t (&r)[8], uint64_t d0, uint64_t d1, uint64_t L) {
  const uint64_t a0 = (uint32_t)d1, a1 = d1 >> 32, b0 = (uint32_t)L, b1 = L >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  uint64_t lo = (mid << 32) | (uint32_t)p00;
  uint64_t hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  lo += d0;
  hi += lo < d0 ? 1u : 0u;
  r[0] = (uint32_t)lo;
  r[1] = (uint32_t)(lo >> 32);
  r[2] = (uint32_t)hi;
  r[3] = (uint32_t)(hi >> 32);
#pragma unroll
  for (int k = 4; k < 8; k++) r[k] = 0;
}
template <class C>
MLHIP_HD void g1_endo_split(uint32_t (&a)[8], uint32_t (&b)[8], const uint32_t (&s)[8]) {
  uint32_t dig[8];
  gt_exp_split<C>(dig, s);
  endo_mac64(a, dig[0] | ((uint64_t)dig[1] << 32), dig[2] | ((uint64_t)dig[3] << 32), GtSplit<C>::LO);
  endo_mac64(b, dig[4] | ((uint64_t)dig[5] << 32), dig[6] | ((uint64_t)dig[7] << 32), GtSplit<C>::LO);
}

// ---- G1 of BN254: the GLV lattice split ----------------------------------------------------------------------------------
// does the promise change the chain of G1 of this curve although ScalarMulEndo<C, true> says no?  (A trait of its own:
// ScalarMulEndo keeps meaning "s = a + b x^2 exists".)
template <class C>
struct G1Glv {
  static constexpr bool AVAILABLE = C::IS_BN;
};

// out[0 .. NA + NB) = a[0 .. NA) * b[0 .. NB), 32-bit limbs (once per product: no need for anything faster)
template <int NA, int NB>
MLHIP_HD void glv_mul_words(uint32_t* out, const uint32_t* a, const uint32_t* b) {
#pragma unroll
  for (int k = 0; k < NA + NB; k++) out[k] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      c += (uint64_t)a[i] * b[j] + out[i + j];
      out[i + j] = (uint32_t)c;
      c >>= 32;
    }
    out[i + NB] = (uint32_t)c;
  }
}
// c = floor((s g + 2^255) / 2^256), four words (below: c < 2^127)
MLHIP_HD void glv_round_quotient(uint32_t (&c)[4], const uint32_t (&s)[8], const uint32_t (&g)[8]) {
  uint32_t t[16];
  glv_mul_words<8, 8>(t, s, g);
  uint64_t cy = (uint64_t)t[7] + 0x80000000u;
  cy >>= 32;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    cy += t[8 + k];
    c[k] = (uint32_t)cy;
    cy >>= 32;
  }
}
// r -= x (eight words, two's complement mod 2^256)
MLHIP_HD void glv_sub8(uint32_t (&r)[8], const uint32_t (&x)[8]) {
  uint64_t br = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t d = (uint64_t)r[k] - x[k] - br;
    r[k] = (uint32_t)d;
    br = (d >> 32) & 1;
  }
}
// the sign of a two's complement value of eight words, which is replaced by its magnitude
MLHIP_HD bool glv_abs8(uint32_t (&r)[8]) {
  const bool neg = (r[7] >> 31) != 0;
  const uint32_t m = neg ? 0xFFFFFFFFu : 0u;
  uint64_t c = neg ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    c += (uint64_t)(r[k] ^ m);
    r[k] = (uint32_t)c;
    c >>= 32;
  }
  return neg;
}

// s = k1 + k2 lambda (mod r) for canonical s < r: a = |k1|, b = |k2| as eight zero-extended words (what signed_windows4
// reads), neg_a / neg_b their signs.  With the basis v1 = (A, -B), v2 = (B, A + B) of the lattice {(x, y): x + y lambda = 0
// mod r} (A = GLV_A1, B = GLV_A2 = |GLV_B1|, A + B = GLV_B2; det = A (A + B) + B^2 = r):
//     (s, 0) = b1 v1 + b2 v2 over the rationals with b1 = s (A + B) / r, b2 = s B / r;
//     c1 = floor((s G1 + 2^255) / 2^256), c2 = floor((s G2 + 2^255) / 2^256), G1 = floor(2^256 (A + B) / r), G2 = floor(2^256 B / r);
//     (k1, k2) = (s, 0) - c1 v1 - c2 v2 = (s - c1 A - c2 B, c1 B - c2 (A + B)),
// and k1 + k2 lambda = s mod r because v1 and v2 lie in the lattice -- whatever c1, c2 are.
// The bound.  G1 > 2^256 (A + B) / r - 1, so s G1 / 2^256 lies in (b1 - s / 2^256, b1], and s < r < 2^254 makes that
// (b1 - 1/4, b1].  c1 = floor(that + 1/2) is then in (b1 - 3/4, b1 + 1/2]: e1 = b1 - c1 lies in [-1/2, 3/4); the same holds
// for e2 = b2 - c2.  (k1, k2) = e1 v1 + e2 v2 = (e1 A + e2 B, -e1 B + e2 (A + B)), so
//     |k1| < 3/4 (A + B),  |k2| < 3/4 (A + 2 B),   A + 2 B < 1.48 * 10^38 + 2 * 10^19 < 2^127 = 1.70 * 10^38:
// |k1|, |k2| < 3/4 * 2^127 < 2^127 for EVERY s < r -- a, b < 2^128 with a bit to spare, so signed_windows4 leaves window 32
// a carry of 0 and the 33 windows of g1_endo_chain hold them.  c1 <= b1 + 1/2 < A + B + 1 and c2 < B + 1 fit four words;
// k1 and k2 are computed mod 2^256 in two's complement, exact because the true values are far inside (-2^255, 2^255).
template <class C>
MLHIP_HD void g1_glv_split(uint32_t (&a)[8], uint32_t (&b)[8], bool& neg_a, bool& neg_b, const uint32_t (&s)[8]) {
  static_assert(!C::GLV_A1_NEG && C::GLV_B1_NEG && !C::GLV_A2_NEG && !C::GLV_B2_NEG, "written for v1 = (A, -B), v2 = (B, A + B)");
  uint32_t c1[4], c2[4], t[8];
  glv_round_quotient(c1, s, C::GLV_G1);
  glv_round_quotient(c2, s, C::GLV_G2);
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = s[k];
  glv_mul_words<4, 4>(t, c1, C::GLV_A1);
  glv_sub8(a, t);
  glv_mul_words<4, 4>(t, c2, C::GLV_A2);
  glv_sub8(a, t);
  glv_mul_words<4, 4>(b, c1, C::GLV_B1);
  glv_mul_words<4, 4>(t, c2, C::GLV_B2);
  glv_sub8(b, t);
  neg_a = glv_abs8(a);
  neg_b = glv_abs8(b);
}

// What g1_endo_chain and the chunks of msm_batch_endo.h run over: [s]P = +-[a]P +- [b]phi(P), phi(x, y) = (beta x, y).
// BLS12: the signs are constants (+a on P, -b on phi(P): s = a + b x^2 and phi = [-x^2]) and the chain is compiled with
// them -- the code it was before BN254 had a split.  BN254: the signs of k1, k2 come with every scalar.
template <class C, bool BN = C::IS_BN>
struct G1Split {
  static constexpr bool FIXED_SIGNS = true;
  MLHIP_HD static void beta(Fp<C>& r) { fp_from_const<C>(r, C::ENDO_BETA); }
  MLHIP_HD static void split(uint32_t (&a)[8], uint32_t (&b)[8], bool& neg_a, bool& neg_b, const uint32_t (&s)[8]) {
    g1_endo_split<C>(a, b, s);
    neg_a = false;
    neg_b = true;
  }
};
template <class C>
struct G1Split<C, true> {
  static constexpr bool FIXED_SIGNS = false;
  MLHIP_HD static void beta(Fp<C>& r) { fp_from_const<C>(r, C::GLV_BETA); }
  MLHIP_HD static void split(uint32_t (&a)[8], uint32_t (&b)[8], bool& neg_a, bool& neg_b, const uint32_t (&s)[8]) {
    g1_glv_split<C>(a, b, neg_a, neg_b, s);
  }
};

// acc = [s]P for P in G1, s < r.  tab[0] = P on entry; tab[1 .. 7] are scratch.  O: the group operations of the
// caller (dbl / add / madd), inline or out of line as its register budget wants.
template <class C, class F, class O>
MLHIP_HD void g1_endo_chain(XYZZ<F>& acc, XYZZ<F> (&tab)[8], const Affine<F>& P, const uint32_t (&s)[8]) {
  typedef G1Split<C> S;
  uint32_t a[8], b[8], wa[9], wb[9];
  bool neg_a, neg_b;
  S::split(a, b, neg_a, neg_b, s);
  signed_windows4(wa, a);  // a, b < 2^128: the digits of windows 0 .. 31, a carry of 0 / 1 in window 32, nothing above
  signed_windows4(wb, b);
#pragma unroll 1
  for (int k = 1; k < 8; k++) {
    tab[k] = tab[k - 1];
    O::madd(tab[k], P);
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
        O::dbl(t, acc);
        acc = t;
      }
    }
#pragma unroll 1
    for (int half = 0; half < 2; half++) {  // a's digit on +-P, then b's digit on +-phi(P) = (beta x, +-y)
      const int d = signed_window4_digit(half ? wb : wa, w);
      if (d) {
        XYZZ<F> q = tab[(d < 0 ? -d : d) - 1];
        typename F::T ny;
        F::neg(ny, q.y);
        const bool neg_half = S::FIXED_SIGNS ? half != 0 : (half ? neg_b : neg_a);
        F::select(q.y, (d < 0) != neg_half, ny, q.y);
        if (half) F::mul(q.x, q.x, beta);
        O::add(acc, q);
        started = true;
      }
    }
  }
}

// psi on an affine point of the twist over either Fp2 shape (one lane: Fp2<C>; lane pair: Fp2L<C>): conjugate, scale.
// (0, 0) stays (0, 0).  neg: the image negated (g_i of a curve with x < 0, odd i).
template <class C, class F>
MLHIP_HD void g2_psi_affine(Affine<F>& r, const Affine<F>& a, bool neg) {
  typename F::T k, t, u, nu;
  fp2_conj<C>(t, a.x);
  fp2_from_const<C>(k, C::PSI_X);
  F::mul(u, t, k);
  fp2_conj<C>(t, a.y);
  r.x = u;
  fp2_from_const<C>(k, C::PSI_Y);
  F::mul(u, t, k);
  F::neg(nu, u);
  F::select(r.y, neg, nu, u);
}

// The 15-entry Straus table of Q in G2 that gt_exp_step_index addresses (index - 1), shared by g2_endo_chain and the chunks
// of msm_batch_endo.h.  Q itself is read once; no branch or address depends on it.
template <class C, class F, class O>
MLHIP_HD void g2_endo_table(XYZZ<F> (&tab)[15], const Affine<F>& Q) {
  xyzz_from_affine<F>(tab[0], Q);
  if constexpr (C::IS_BN) {
    // tab[a + 4 b - 1] = [a]Q + [b]psi(Q), a, b in 0 .. 3
    Affine<F> g;
    g2_psi_affine<C, F>(g, Q, false);
    xyzz_from_affine<F>(tab[3], g);
    O::dbl(tab[1], tab[0]);
    tab[2] = tab[1];
    O::add(tab[2], tab[0]);
    O::dbl(tab[7], tab[3]);
    tab[11] = tab[7];
    O::add(tab[11], tab[3]);
#pragma unroll 1
    for (int b = 1; b < 4; b++)
#pragma unroll 1
      for (int a = 0; a < 3; a++) {
        tab[4 * b + a] = tab[a];
        O::add(tab[4 * b + a], tab[4 * b - 1]);
      }
  } else {
    // tab[m - 1] = sum over the bits i of m of g_i, g_i = psi^i(Q), negated for odd i when x < 0 (psi = [x] = -[|x|])
    Affine<F> g, h;
    g2_psi_affine<C, F>(g, Q, false);  // psi(Q)
    g2_psi_affine<C, F>(h, g, false);  // psi^2(Q)
    xyzz_from_affine<F>(tab[3], h);
    g2_psi_affine<C, F>(h, h, C::X_NEG);  // +-psi^3(Q)
    xyzz_from_affine<F>(tab[7], h);
    if (C::X_NEG) F::neg(g.y, g.y);
    xyzz_from_affine<F>(tab[1], g);
#pragma unroll 1
    for (int top = 1; top < 4; top++) {
      const int base = 1 << top;  // tab[base - 1] = g_top
#pragma unroll 1
      for (int k = 0; k < base - 1; k++) {
        tab[base + k] = tab[k];
        O::add(tab[base + k], tab[base - 1]);
      }
    }
  }
}

// acc = [s]Q for Q in G2, dig = gt_exp_split(s), s < r.  tab is scratch.  Every branch depends on the scalar alone: uniform
// over the two lanes of a product.
template <class C, class F, class O>
MLHIP_HD void g2_endo_chain(XYZZ<F>& acc, XYZZ<F> (&tab)[15], const Affine<F>& Q, const uint32_t (&dig)[8]) {
  g2_endo_table<C, F, O>(tab, Q);
  constexpr int DBL = C::IS_BN ? 2 : 1;
  xyzz_set_inf<F>(acc);
  bool started = false;
#pragma unroll 1
  for (int j = 63; j >= 0; j--) {
    if (started) {
#pragma unroll 1
      for (int d = 0; d < DBL; d++) {
        XYZZ<F> t;
        O::dbl(t, acc);
        acc = t;
      }
    }
    const uint32_t m = gt_exp_step_index<C>(dig, j);
    if (m) {
      if (started)
        O::add(acc, tab[m - 1]);
      else {
        acc = tab[m - 1];
        started = true;
      }
    }
  }
}

#if defined(__HIPCC__)
// ---- the kernels: the loads, stores and launch shapes of k_scalar_mul / k_scalar_mul_lp ------------------------------
template <class C>
struct EndoOpsG1 {  // the running point stays in registers (k_scalar_mul's kInline)
  typedef FpField<C> F;
  __device__ static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
  __device__ static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  __device__ static void madd(XYZZ<F>& acc, const Affine<F>& q) { xyzz_madd_ool<F>(acc, q); }
};
template <class C>
struct EndoOpsG2Lp {
  typedef Fp2LField<C> F;
  __device__ static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
  __device__ static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add_lp_ool<C>(acc, q); }
};

// out[i] = [s_i] P_i, P_i in G1 (BLS12: the subgroup; BN254: the curve): one lane per product
template <class C>
__global__ void __launch_bounds__(64) k_scalar_mul_endo(const Affine<FpField<C>>* __restrict__ points, size_t point_stride,
                                                        const uint32_t* __restrict__ scalars, int mont, size_t n,
                                                        Affine<FpField<C>>* __restrict__ out) {
  typedef FpField<C> F;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
  fr_canonical<C>(s, scalars + 8 * i, mont != 0);
  const Affine<F> P = points[i * point_stride];
  XYZZ<F> tab[8];
  xyzz_from_affine<F>(tab[0], P);
  XYZZ<F> acc;
  g1_endo_chain<C, F, EndoOpsG1<C>>(acc, tab, P, s);
  Affine<F> r;
  xyzz_to_affine<F>(r, acc);
  out[i] = r;
}

// out[i] = [s_i] Q_i, Q_i in G2: one lane pair per product (k_scalar_mul_lp), the 15-entry table in scratch
template <class C>
__global__ void __launch_bounds__(64) k_scalar_mul_endo_lp(const Affine<Fp2Field<C>>* __restrict__ points, size_t point_stride,
                                                           const uint32_t* __restrict__ scalars, int mont, size_t n,
                                                           Affine<Fp2Field<C>>* __restrict__ out) {
  typedef Fp2LField<C> FL;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 1;  // both lanes of a pair share i and the scalar: every branch below is pair-uniform
  if (i >= n) return;
  const int hi = (int)(threadIdx.x & 1u);
  uint32_t s[8], dig[8];
  fr_canonical<C>(s, scalars + 8 * i, mont != 0);
  gt_exp_split<C>(dig, s);
  Affine<FL> Q;
  lp_load_affine<C>(Q, points, i * point_stride, hi);
  XYZZ<FL> tab[15];
  XYZZ<FL> acc;
  g2_endo_chain<C, FL, EndoOpsG2Lp<C>>(acc, tab, Q, dig);
  Affine<FL> r;
  xyzz_to_affine<FL>(r, acc);
  Fp<C>* o = reinterpret_cast<Fp<C>*>(out + i);
  o[hi] = r.x.v;
  o[2 + hi] = r.y.v;
}

// MLHIP_SCALAR_MUL_ENDO=0: every promised call on the plain kernels (second implementation, A/B)
static inline bool scalar_mul_endo_enabled() {
  const char* e = getenv("MLHIP_SCALAR_MUL_ENDO");
  return !(e && e[0] == '0');
}

// the promised products of scalar_mul_device (msm_scalar_mul.h), below its fixed-base table path; false: not for this
// (curve, group) -- the caller goes on to the plain kernel
template <class C, class F>
bool scalar_mul_endo_launch(const void* d_points, size_t point_stride, const void* d_scalars, int mont, size_t n, void* d_out,
                            hipStream_t st) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  if constexpr (!ScalarMulEndo<C, kG1>::AVAILABLE && !(kG1 && G1Glv<C>::AVAILABLE)) {
    return false;
  } else {
    if (!scalar_mul_endo_enabled()) return false;
    if constexpr (kG1)
      k_scalar_mul_endo<C><<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>((const Affine<F>*)d_points, point_stride,
                                                                               (const uint32_t*)d_scalars, mont, n, (Affine<F>*)d_out);
    else
      k_scalar_mul_endo_lp<C><<<dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, st>>>((const Affine<F>*)d_points, point_stride,
                                                                                     (const uint32_t*)d_scalars, mont, n,
                                                                                     (Affine<F>*)d_out);
    return true;
  }
}
#endif  // __HIPCC__

}  // namespace mlhip
