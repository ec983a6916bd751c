// pairing_prepared.h -- Miller loops against FIXED G2 points ("G2Prepared"): the line coefficients of the optimal-ate
// loop depend on Q alone, so they are computed once per Q (g2_prepare_lines), kept on the device, and the loop that
// consumes them (miller_loop_prepared_core / _q) carries no point T at all -- per pair and iteration it is the two
// Fp2 x Fp products of mul_by_line and the sparse Fp12 product.
//
// Serves the reference's verifier shape: Pairing2(g, sig, pk, h) + FExp with both G2 arguments the same in every call
// (driver/gurvy/bls12381/bls12-381.go:448-468, bn254.go:247-267, bls12-377.go:244-264).
//
// The lines are produced by pairing.h's own g2_double_step / g2_add_step in pairing.h's order (for BN254 with the two
// Frobenius lines at the end), so the prepared loop multiplies the same field elements into f as miller_loop_core does:
// final_exp of the two is byte-identical, for any Q on the curve (in the subgroup or not).
//
// Table layout.  A Q owns prepared_num_lines<C>() lines in loop order (doubling line of iteration i, then its addition
// line if the bit is set).  Two images of a line exist:
//   * boundary form: Line<C, Fp2<C>> (canonical Montgomery values, 32-bit limbs) -- the one-lane kernel of the test build and the host model;
//   * carry-free form: int32 [r0 r1 r2][c0 c1][N28] -- fp28_from_fp of the above, i.e. normalized (weight 1, value < p):
//     a lane of the lane-pair / quad kernels reads the three N28-limb strings of ITS Fp2 component and multiplies them as they are.
#pragma once
#include "fp2_lanes28.h"
#include "pairing.h"
#include "pairing_quad.h"

namespace mlhip {

// doubling lines + addition lines (+ BN254's two Frobenius lines)
template <class C>
constexpr int prepared_num_lines() {
  int n = 0;
  for (int i = C::ATE_BITS - 2; i >= 0; i--) {
    const bool bit = (i >= 64) ? ((C::ATE_HI >> (i - 64)) & 1) : ((C::ATE_LO >> i) & 1);
    n += bit ? 2 : 1;
  }
  return n + (C::IS_BN ? 2 : 0);
}

// int32 words of one Q's carry-free table
template <class C>
constexpr size_t prepared_words28() {
  return (size_t)prepared_num_lines<C>() * 6 * C::N28;
}

// sink(li, line): every line of Q = (qx, qy) in loop order, li = 0 .. prepared_num_lines - 1.  Q at infinity (0, 0) or off
// the curve runs the same straight-line arithmetic on whatever it is given.
template <class C, class Sink>
MLHIP_HD void g2_prepare_lines(const Fp2<C>& qx, const Fp2<C>& qy, Sink& sink) {
  typedef Fp2<C> E2;
  G2Proj<C, E2> T;
  T.x = qx;
  T.y = qy;
  fp2_one<C>(T.z);
  Line<C, E2> l;
  int li = 0;
#pragma unroll 1
  for (int i = C::ATE_BITS - 2; i >= 0; i--) {
    const bool bit = (i >= 64) ? ((C::ATE_HI >> (i - 64)) & 1) : ((C::ATE_LO >> i) & 1);
    g2_double_step<C>(T, l);
    sink(li++, l);
    if (bit) {
      g2_add_step<C>(T, qx, qy, l);
      sink(li++, l);
    }
  }
  if constexpr (C::IS_BN) {
    // lines through pi(Q) and -pi^2(Q) (miller_loop_core's tail)
    E2 x1, y1, x2, y2, g;
    fp2_conj<C>(x1, qx);
    fp2_from_const<C>(g, C::GAMMA1[2]);
    fp2_mul<C>(x1, x1, g);
    fp2_conj<C>(y1, qy);
    fp2_from_const<C>(g, C::GAMMA1[3]);
    fp2_mul<C>(y1, y1, g);
    fp2_mul_by_real_const<C>(x2, qx, C::GAMMA2[2]);
    fp2_mul_by_real_const<C>(y2, qy, C::GAMMA2[3]);
    fp2_neg<C>(y2, y2);
    g2_add_step<C>(T, x1, y1, l);
    sink(li++, l);
    g2_add_step<C>(T, x2, y2, l);
    sink(li++, l);
  }
}

// one boundary-form line -> its 6 N28 words of the carry-free image
template <class C>
MLHIP_HD void prepared_line_to28(int32_t* w, const Line<C, Fp2<C>>& l) {
  const Fp<C>* c[6] = {&l.r0.c0, &l.r0.c1, &l.r1.c0, &l.r1.c1, &l.r2.c0, &l.r2.c1};
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fp28<C> t;
    fp28_from_fp<C>(t, *c[k]);
#pragma unroll
    for (int i = 0; i < C::N28; i++) w[k * C::N28 + i] = t.l[i];
  }
}

// f = prod_k f_{loop,Q_k}(P_k) with the lines of pair k read through ls.load(line, k, li) -- miller_loop_core without the
// G2 arithmetic: the shared squaring rides with the iteration's first live line, pairs that are not live (either side at
// infinity) are skipped.
template <class C, int MAXP, class E2, class EP, class LS>
MLHIP_HD void miller_loop_prepared_core(Fp12<C, E2>& f, const EP* px, const EP* py, const bool* live, int n_pairs,
                                        const LS& ls) {
  int any = 0;
  for (int k = 0; k < n_pairs && k < MAXP; k++) any |= live[k];
  fp12_one<C>(f);
  if (!any) return;
  Line<C, E2> l;
  bool first = true;
  int li = 0;
#pragma unroll 1
  for (int i = C::ATE_BITS - 2; i >= 0; i--) {
    bool square = !first;
    first = false;
    const bool bit = (i >= 64) ? ((C::ATE_HI >> (i - 64)) & 1) : ((C::ATE_LO >> i) & 1);
    for (int k = 0; k < n_pairs && k < MAXP; k++) {
      if (!live[k]) continue;
      ls.load(l, k, li);
      if (square)
        sqr_mul_by_line<C>(f, l, px[k], py[k]);
      else
        mul_by_line<C>(f, l, px[k], py[k]);
      square = false;
      if (bit) {
        ls.load(l, k, li + 1);
        mul_by_line<C>(f, l, px[k], py[k]);
      }
    }
    li += bit ? 2 : 1;
  }
  if constexpr (C::IS_BN) {
    for (int k = 0; k < n_pairs && k < MAXP; k++) {
      if (!live[k]) continue;
      ls.load(l, k, li);
      mul_by_line<C>(f, l, px[k], py[k]);
      ls.load(l, k, li + 1);
      mul_by_line<C>(f, l, px[k], py[k]);
    }
  }
  if (C::X_NEG) fp12_conj<C>(f, f);
}

// the same on a quad of lanes (pairing_quad.h: miller_loop_q without the G2 arithmetic); the lines are replicated on both pairs
template <class C, int MAXP, class E, class EP, class LS>
MLHIP_HD void miller_loop_prepared_q(Fp12Q<C, E>& f, const EP* px, const EP* py, const bool* live, int n_pairs,
                                     const LS& ls) {
  int any = 0;
  for (int k = 0; k < n_pairs && k < MAXP; k++) any |= live[k];
  fp12q_one<C>(f);
  if (!any) return;
  Line<C, E> l;
  bool first = true;
  int li = 0;
#pragma unroll 1
  for (int i = C::ATE_BITS - 2; i >= 0; i--) {
    if (!first) fp12q_sqr<C>(f, f);
    first = false;
    const bool bit = (i >= 64) ? ((C::ATE_HI >> (i - 64)) & 1) : ((C::ATE_LO >> i) & 1);
    for (int k = 0; k < n_pairs && k < MAXP; k++) {
      if (!live[k]) continue;
      ls.load(l, k, li);
      mul_by_line_q<C>(f, l, px[k], py[k]);
      if (bit) {
        ls.load(l, k, li + 1);
        mul_by_line_q<C>(f, l, px[k], py[k]);
      }
    }
    li += bit ? 2 : 1;
  }
  if constexpr (C::IS_BN) {
    for (int k = 0; k < n_pairs && k < MAXP; k++) {
      if (!live[k]) continue;
      ls.load(l, k, li);
      mul_by_line_q<C>(f, l, px[k], py[k]);
      ls.load(l, k, li + 1);
      mul_by_line_q<C>(f, l, px[k], py[k]);
    }
  }
  if (C::X_NEG) fp12q_conj<C>(f, f);
}

// ---- line sources ---------------------------------------------------------------------------------------------------------
// boundary-form table: Line<C, Fp2<C>> [m][NL]; q[k] = which Q slot k of every product pairs with
template <class C>
struct PreparedLines32 {
  const Line<C, Fp2<C>>* tab;
  uint32_t q[4];
  MLHIP_HD void load(Line<C, Fp2<C>>& l, int k, int li) const { l = tab[(size_t)q[k] * prepared_num_lines<C>() + li]; }
};

}  // namespace mlhip
