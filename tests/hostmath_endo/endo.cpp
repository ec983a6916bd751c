// TEST ARTIFACT -- host (g++) build of msm_scalar_mul_endo.h, loaded by tests/test_scalar_mul_subgroup_host.py through ctypes
// and compared with Python integers and oracle/pyref.py: the compiled endomorphism constants applied to a point, the scalar
// split, and the whole G1 and G2 chains of the kernels behind MLHIP_GROUP_SUBGROUP on the one-lane field types (the
// kernels run the same templates on FpField / the lane-pair Fp2).  It is NOT part of libmlhip.so.
#include <stdint.h>
#include <string.h>
#include "../../mathlib_amd/csrc/msm_scalar_mul_endo.h"

using namespace mlhip;

template <class F>
struct HostOps {
  static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
  static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  static void madd(XYZZ<F>& acc, const Affine<F>& q) { xyzz_madd<F>(acc, q, false); }
};

template <class C>
struct Ex {
  typedef FpField<C> F1;
  typedef Fp2Field<C> F2;

  // (beta x, -y) of a G1 point through the compiled ENDO_BETA: what the chain adds for a digit +1 of b
  static int phi_neg(const void* in, void* out) {
    if (C::IS_BN) return -3;
    Affine<F1> p;
    memcpy(&p, in, sizeof(p));
    Fp<C> beta;
    fp_from_const<C>(beta, C::ENDO_BETA);
    F1::mul(p.x, p.x, beta);
    F1::neg(p.y, p.y);
    memcpy(out, &p, sizeof(p));
    return 0;
  }
  // psi of a G2 point through the compiled PSI_X / PSI_Y
  static int psi(const void* in, void* out) {
    Affine<F2> q, r;
    memcpy(&q, in, sizeof(q));
    g2_psi_affine<C, F2>(r, q, false);
    memcpy(out, &r, sizeof(r));
    return 0;
  }
  // behind fr_canonical (mont < 0: the value as it is): a, b of the G1 split (BLS12), the digits of the G2 split
  static int split(const uint32_t* scalar, int mont, uint32_t* a_out, uint32_t* b_out, uint32_t* dig_out, uint32_t* canon_out) {
    uint32_t s[8], a[8], b[8], dig[8];
    if (mont < 0)
      memcpy(s, scalar, sizeof(s));
    else
      fr_canonical<C>(s, scalar, mont != 0);
    memset(a, 0, sizeof(a));
    memset(b, 0, sizeof(b));
    if (!C::IS_BN) g1_endo_split<C>(a, b, s);
    gt_exp_split<C>(dig, s);
    memcpy(a_out, a, sizeof(a));
    memcpy(b_out, b, sizeof(b));
    memcpy(dig_out, dig, sizeof(dig));
    memcpy(canon_out, s, sizeof(s));
    return GtSplit<C>::DIM;
  }
  static int g1_mul(const void* in, const uint32_t* scalar, int mont, void* out) {
    if (C::IS_BN) return -3;
    Affine<F1> p, r;
    memcpy(&p, in, sizeof(p));
    uint32_t s[8];
    fr_canonical<C>(s, scalar, mont != 0);
    XYZZ<F1> tab[8], acc;
    xyzz_from_affine<F1>(tab[0], p);
    g1_endo_chain<C, F1, HostOps<F1>>(acc, tab, p, s);
    xyzz_to_affine<F1>(r, acc);
    memcpy(out, &r, sizeof(r));
    return 0;
  }
  static int g2_mul(const void* in, const uint32_t* scalar, int mont, void* out) {
    Affine<F2> q, r;
    memcpy(&q, in, sizeof(q));
    uint32_t s[8], dig[8];
    fr_canonical<C>(s, scalar, mont != 0);
    gt_exp_split<C>(dig, s);
    XYZZ<F2> tab[15], acc;
    g2_endo_chain<C, F2, HostOps<F2>>(acc, tab, q, dig);
    xyzz_to_affine<F2>(r, acc);
    memcpy(out, &r, sizeof(r));
    return 0;
  }
};

#define EX_DISPATCH(call)                  \
  switch (curve) {                         \
    case 0: return Ex<Bn254>::call;        \
    case 1: return Ex<Bls381>::call;       \
    case 2: return Ex<Bls377>::call;       \
    default: return -2;                    \
  }

extern "C" {
// does MLHIP_GROUP_SUBGROUP change the chain of this (curve, group)?
int ex_available(int curve, int group) {
  switch (curve) {
    case 0: return group == 1 ? ScalarMulEndo<Bn254, true>::AVAILABLE : ScalarMulEndo<Bn254, false>::AVAILABLE;
    case 1: return group == 1 ? ScalarMulEndo<Bls381, true>::AVAILABLE : ScalarMulEndo<Bls381, false>::AVAILABLE;
    case 2: return group == 1 ? ScalarMulEndo<Bls377, true>::AVAILABLE : ScalarMulEndo<Bls377, false>::AVAILABLE;
    default: return -2;
  }
}
int ex_phi_neg(int curve, const void* in, void* out) { EX_DISPATCH(phi_neg(in, out)) }
int ex_psi(int curve, const void* in, void* out) { EX_DISPATCH(psi(in, out)) }
int ex_split(int curve, const uint32_t* scalar, int mont, uint32_t* a, uint32_t* b, uint32_t* dig, uint32_t* canon) {
  EX_DISPATCH(split(scalar, mont, a, b, dig, canon))
}
int ex_g1_mul(int curve, const void* in, const uint32_t* scalar, int mont, void* out) { EX_DISPATCH(g1_mul(in, scalar, mont, out)) }
int ex_g2_mul(int curve, const void* in, const uint32_t* scalar, int mont, void* out) { EX_DISPATCH(g2_mul(in, scalar, mont, out)) }
}
