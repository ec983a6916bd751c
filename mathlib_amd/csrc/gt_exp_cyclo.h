// gt_exp_cyclo.h -- the chains of Gt.Exp over the two shapes of a Gt value (GtOpsLp, GtOpsQ): the 4-bit windowed chain behind
// mlhip_gt_exp, valid for any Fp12 value, and, for MEMBERS of Gt (the subgroup of order r of Fp12*), the scalar split and the
// chain behind mlhip_gt_exp_cyclo.  Included by pairing_kernels.h; host-testable (tests/hostmath_gtexp).
//
// On Gt the Frobenius map f -> f^p is exponentiation by p mod r, and members of Gt lie in the cyclotomic subgroup, where a
// squaring is the Granger-Scott one (nine Fp2 squarings) and the inverse is the conjugate.  So f^s is computed as
//     BLS12 (p = x mod r, |x| < 2^64 < r^(1/4)):   s = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3,   f^s = prod g_i^(d_i),
//                                                  g_i = frob^i(f), conjugated for odd i when x < 0
//     BN254 (p = 6 x^2 =: L mod r, L < 2^127, L^2 < r):   s = d0 + d1 L,   f^s = f^(d0) frob(f)^(d1)
// with one shared chain of 64 steps over a 15-entry table of products of the g_i (Straus): 64 cyclotomic squarings (BN254:
// 128) and at most 75 (77) products instead of 255 generic squarings and at most 78 products.  An input outside Gt gives a
// wrong value and nothing else: every operation is straight-line field arithmetic.
#pragma once
#include "msm_body.h"
#include "pairing_quad.h"

namespace mlhip {

// the modulus of the split as two 64-bit halves: |x| (BLS12) or 6 x^2 (BN254)
template <class C>
struct GtSplit {
  static constexpr unsigned __int128 L = C::IS_BN ? (unsigned __int128)6 * C::X_ABS * C::X_ABS : (unsigned __int128)C::X_ABS;
  static constexpr uint64_t LO = (uint64_t)L, HI = (uint64_t)(L >> 64);
  static constexpr int DIM = C::IS_BN ? 2 : 4;        // digits
  static constexpr int DIGIT_WORDS = C::IS_BN ? 4 : 2;  // 32-bit words per digit
  static_assert(HI < ((uint64_t)1 << 63), "the restoring division shifts its remainder left by one bit");
  static_assert(C::IS_BN || HI == 0, "BLS12: the seed is a 64-bit value");
};

// q = floor(n / d), rem = n mod d for a 256-bit n and d = dh 2^64 + dl < 2^127: plain restoring division, one bit per
// step, branch-free (the lanes of a wave hold different scalars)
MLHIP_HD void gt_divmod256(uint32_t (&q)[8], uint64_t& rem_lo, uint64_t& rem_hi, const uint32_t (&n)[8], uint64_t dl, uint64_t dh) {
  uint64_t l = 0, h = 0;
#pragma unroll
  for (int w = 7; w >= 0; w--) {
    const uint32_t nw = n[w];
    uint32_t qw = 0;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      h = (h << 1) | (l >> 63);
      l = (l << 1) | (uint64_t)((nw >> b) & 1u);
      const uint64_t sl = l - dl, sh = h - dh - (l < dl ? 1u : 0u);
      const bool ge = h > dh || (h == dh && l >= dl);
      l = ge ? sl : l;
      h = ge ? sh : h;
      qw = (qw << 1) | (ge ? 1u : 0u);
    }
    q[w] = qw;
  }
  rem_lo = l;
  rem_hi = h;
}

// the digits of a scalar s < r (fr_canonical's output): dig[DIGIT_WORDS i ..] = d_i, little-endian words.  The LAST digit
// is the remaining quotient, not reduced again: below 2^64 on the BLS12 curves (r < x^4), below 2^127 on BN254 -- where it
// exceeds L for s close to r (s = r - 1: d1 = L + ...), so a third digit would appear if it were.
template <class C>
MLHIP_HD void gt_exp_split(uint32_t (&dig)[8], const uint32_t (&s)[8]) {
  typedef GtSplit<C> S;
  uint32_t n[8], q[8];
#pragma unroll
  for (int i = 0; i < 8; i++) n[i] = s[i];
#pragma unroll
  for (int k = 0; k < S::DIM - 1; k++) {
    uint64_t rl, rh;
    gt_divmod256(q, rl, rh, n, S::LO, S::HI);
    dig[S::DIGIT_WORDS * k] = (uint32_t)rl;
    dig[S::DIGIT_WORDS * k + 1] = (uint32_t)(rl >> 32);
    if (S::DIGIT_WORDS == 4) {
      dig[S::DIGIT_WORDS * k + 2] = (uint32_t)rh;
      dig[S::DIGIT_WORDS * k + 3] = (uint32_t)(rh >> 32);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) n[i] = q[i];
  }
#pragma unroll
  for (int i = 0; i < S::DIGIT_WORDS; i++) dig[S::DIGIT_WORDS * (S::DIM - 1) + i] = n[i];
}

// the table index of step j (63 .. 0), 0 = no product.  BLS12: bit j of the four digits; BN254: bits 2j+1, 2j of d0 (a) and
// of d1 (b), index a + 4 b.
template <class C>
MLHIP_HD uint32_t gt_exp_step_index(const uint32_t (&dig)[8], int j) {
  if (C::IS_BN) {
    const int b = 2 * j;
    const uint32_t a0 = (dig[b >> 5] >> (b & 31)) & 3u, a1 = (dig[4 + (b >> 5)] >> (b & 31)) & 3u;
    return a0 | (a1 << 2);
  }
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) m |= ((dig[2 * i + (j >> 5)] >> (j & 31)) & 1u) << i;
  return m;
}

// ---- the two shapes of a Gt value the chain runs on ---------------------------------------------------------------------
// lane pairs (tower.h): the Fp12 of one exponentiation on two lanes, or on one with the boundary-form element
template <class C, class E>
struct GtOpsLp {
  typedef Fp12<C, E> T;
  static MLHIP_HD void one(T& r) { fp12_one<C>(r); }
  static MLHIP_HD void mul(T& r, const T& a, const T& b) { fp12_mul<C>(r, a, b); }
  static MLHIP_HD void sqr(T& r, const T& a) { fp12_sqr<C>(r, a); }
  static MLHIP_HD void cyclo_sqr(T& r, const T& a) { fp12_cyclo_sqr<C>(r, a); }
  static MLHIP_HD void conj(T& r, const T& a) { fp12_conj<C>(r, a); }
  template <int K>
  static MLHIP_HD void frob(T& r, const T& a) {
    fp12_frob<C, K>(r, a);
  }
  // what the membership test and Gt.Inverse add (gt_codec.h): the inverse of any Fp12 value, the Fp2 coefficients as an
  // array, and how many lanes share one value on the device (a verdict is combined over them)
  static MLHIP_HD void inv(T& r, const T& a) { fp12_inv<C>(r, a); }
  static constexpr int COEFFS = 6, DEVICE_LANES = 2;
  static MLHIP_HD const E* coeffs(const T& a) { return &a.c0.c0; }
};
// quads (pairing_quad.h): pair A holds the c0 half, pair B the c1 half
template <class C, class E>
struct GtOpsQ {
  typedef Fp12Q<C, E> T;
  static MLHIP_HD void one(T& r) { fp12q_one<C>(r); }
  static MLHIP_HD void mul(T& r, const T& a, const T& b) { fp12q_mul<C>(r, a, b); }
  static MLHIP_HD void sqr(T& r, const T& a) { fp12q_sqr<C>(r, a); }
  static MLHIP_HD void cyclo_sqr(T& r, const T& a) { fp12q_cyclo_sqr<C>(r, a); }
  static MLHIP_HD void conj(T& r, const T& a) { fp12q_conj<C>(r, a); }
  template <int K>
  static MLHIP_HD void frob(T& r, const T& a) {
    fp12q_frob<C, K>(r, a);
  }
  static MLHIP_HD void inv(T& r, const T& a) { fp12q_inv<C>(r, a); }
  static constexpr int COEFFS = 3, DEVICE_LANES = 4;
  static MLHIP_HD const E* coeffs(const T& a) { return &a.v.c0; }
};

// acc = tab[0]^s for ANY Fp12 value tab[0] (raw Miller-loop outputs included, like gnark's GT.Exp) and s < 2^256: 4-bit
// fixed windows.  tab[1 .. 14] become base^2 .. base^15 (in scratch on the device: 4.3 KB per lane, one 288-byte read per
// window), then 4 generic squarings and at most one product per window -- 255 squarings + <= 78 products instead of ~128.
// `acc` is a reference so that a kernel can keep it where it likes (k_gt_exp_lp: an LDS slot).  Every branch depends on the
// scalar only: uniform over the lanes of one exponentiation.
template <class C, class G>
MLHIP_HD void gt_exp_window_chain(typename G::T& acc, typename G::T (&tab)[15], const uint32_t (&s)[8]) {
#pragma unroll 1
  for (int k = 1; k < 15; k++) G::mul(tab[k], tab[k - 1], tab[0]);
  G::one(acc);
  bool started = false;
#pragma unroll 1
  for (int w = 63; w >= 0; w--) {
    if (started) {
#pragma unroll 1
      for (int d = 0; d < 4; d++) G::sqr(acc, acc);
    }
    const uint32_t nib = (s[w >> 3] >> ((w & 7) * 4)) & 15u;
    if (nib) {
      if (started)
        G::mul(acc, acc, tab[nib - 1]);
      else {
        acc = tab[nib - 1];
        started = true;
      }
    }
  }
}

// acc = tab[0]^s for tab[0] in Gt, dig = gt_exp_split(s).  tab[1 .. 14] are scratch: the table has the footprint of the
// generic kernels' 15 powers.  Every branch depends on the scalar only: uniform over the lanes of one exponentiation.
template <class C, class G>
MLHIP_HD void gt_exp_cyclo_chain(typename G::T& acc, typename G::T (&tab)[15], const uint32_t (&dig)[8]) {
  typedef typename G::T T;
  if constexpr (C::IS_BN) {
    // tab[a + 4 b - 1] = f^a frob(f)^b, a, b in 0 .. 3 (the two squares are generic products: one call site less)
    G::template frob<1>(tab[3], tab[0]);
    G::mul(tab[1], tab[0], tab[0]);
    G::mul(tab[2], tab[1], tab[0]);
    G::mul(tab[7], tab[3], tab[3]);
    G::mul(tab[11], tab[7], tab[3]);
#pragma unroll 1
    for (int b = 1; b < 4; b++)
#pragma unroll 1
      for (int a = 0; a < 3; a++) G::mul(tab[4 * b + a], tab[a], tab[4 * b - 1]);
  } else {
    // tab[m - 1] = prod over the bits i of m of g_i
    G::template frob<1>(tab[1], tab[0]);
    G::template frob<2>(tab[3], tab[0]);
    G::template frob<3>(tab[7], tab[0]);
    if (C::X_NEG) {  // p = -|x| mod r: g_1 and g_3 are inverses of the Frobenius images, and the inverse is the conjugate
      G::conj(tab[1], tab[1]);
      G::conj(tab[7], tab[7]);
    }
#pragma unroll 1
    for (int top = 1; top < 4; top++) {
      const int base = 1 << top;  // tab[base - 1] = g_top
#pragma unroll 1
      for (int k = 0; k < base - 1; k++) G::mul(tab[base + k], tab[k], tab[base - 1]);
    }
  }
  constexpr int SQ = C::IS_BN ? 2 : 1;
  G::one(acc);
  bool started = false;
#pragma unroll 1
  for (int j = 63; j >= 0; j--) {
    if (started) {
#pragma unroll 1
      for (int d = 0; d < SQ; d++) G::cyclo_sqr(acc, acc);
    }
    const uint32_t m = gt_exp_step_index<C>(dig, j);
    if (m) {
      if (started)
        G::mul(acc, acc, tab[m - 1]);
      else {
        acc = tab[m - 1];
        started = true;
      }
    }
  }
}

}  // namespace mlhip
