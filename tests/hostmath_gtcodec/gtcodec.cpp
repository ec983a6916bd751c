// TEST ARTIFACT -- host (g++) build of gt_codec.h's membership chain and of the Fp12 inverses behind mlhip_gt_is_member and
// mlhip_gt_inverse, loaded by tests/test_gt_codec_host.py through ctypes and compared with oracle/pyref.py: over the plain
// tower (tower.h on Fp2<C>) and through the host models of the carry-free lane pair and quad (every operation checks its
// weight and value budget and aborts when one is exceeded).  It is NOT part of libmlhip.so.
#include <stdint.h>
#include <string.h>
#include "../../mathlib_amd/csrc/gt_codec.h"

using namespace mlhip;

// the plain tower as a third shape of the chain: the same formulas on saturated limbs, one value per "lane"
template <class C>
struct GtOpsPlain {
  typedef Fp2<C> E;
  typedef Fp12<C> T;
  static void mul(T& r, const T& a, const T& b) { fp12_mul<C>(r, a, b); }
  static void cyclo_sqr(T& r, const T& a) { fp12_cyclo_sqr<C>(r, a); }
  static void conj(T& r, const T& a) { fp12_conj<C>(r, a); }
  template <int K>
  static void frob(T& r, const T& a) {
    fp12_frob<C, K>(r, a);
  }
  static void inv(T& r, const T& a) { fp12_inv<C>(r, a); }
};
// (the saturated form is canonical: the comparisons of the chain are limb comparisons)
template <class C>
bool plain_is_member(const Fp12<C>& f) {
  typedef GtOpsPlain<C> G;
  Fp12<C> a, b, c, zero;
  memset(&zero, 0, sizeof(zero));
  G::template frob<2>(a, f);
  G::template frob<2>(b, a);
  G::mul(c, b, f);
  const bool cyclotomic = fp12_eq<C>(c, a);
  const bool nonzero = !fp12_eq<C>(f, zero);
  gt_pow_seed<C, G>(c, f);
  if constexpr (C::IS_BN) {
    gt_pow_seed<C, G>(b, c);
    G::cyclo_sqr(c, b);
    G::cyclo_sqr(b, c);
    G::mul(c, c, b);
  } else if (C::X_NEG) {
    G::conj(c, c);
  }
  G::template frob<1>(a, f);
  return nonzero & cyclotomic & fp12_eq<C>(c, a);
}

template <class C>
struct Gc {
  typedef Fp2H28<C> EH;
  typedef Fp2Q28H<C> EQ;

  static void load_lp(Fp12<C, EH>& f, const Fp12<C>& in) {
    const Fp2<C>* s = &in.c0.c0;
    EH* d = &f.c0.c0;
    for (int i = 0; i < 6; i++) {
      fp28_from_fp<C>(d[i].c[0], s[i].c0);
      fp28_from_fp<C>(d[i].c[1], s[i].c1);
      d[i].wt = 1;
      d[i].vbound = 1;
    }
  }
  static void store_lp(Fp12<C>& out, const Fp12<C, EH>& f) {
    Fp2<C>* d = &out.c0.c0;
    const EH* s = &f.c0.c0;
    for (int i = 0; i < 6; i++) {
      fp28_to_fp<C>(d[i].c0, s[i].c[0]);
      fp28_to_fp<C>(d[i].c1, s[i].c[1]);
    }
  }
  static void load_q(Fp12Q<C, EQ>& f, const Fp12<C>& in) {
    const Fp2<C>* lo = &in.c0.c0;
    const Fp2<C>* up = &in.c1.c0;
    EQ* d = &f.v.c0;
    for (int j = 0; j < 3; j++) {
      fp28_from_fp<C>(d[j].c[0], lo[j].c0);
      fp28_from_fp<C>(d[j].c[1], lo[j].c1);
      fp28_from_fp<C>(d[j].c[2], up[j].c0);
      fp28_from_fp<C>(d[j].c[3], up[j].c1);
      d[j].wt = 1;
      d[j].vbound = 1;
    }
  }
  static void store_q(Fp12<C>& out, const Fp12Q<C, EQ>& f) {
    Fp2<C>* lo = &out.c0.c0;
    Fp2<C>* up = &out.c1.c0;
    const EQ* s = &f.v.c0;
    for (int j = 0; j < 3; j++) {
      fp28_to_fp<C>(lo[j].c0, s[j].c[0]);
      fp28_to_fp<C>(lo[j].c1, s[j].c[1]);
      fp28_to_fp<C>(up[j].c0, s[j].c[2]);
      fp28_to_fp<C>(up[j].c1, s[j].c[3]);
    }
  }

  // form 0: plain tower, 1: lane-pair model, 2: quad model.  1: in Gt, 0: not (the models abort on a budget violation)
  static int is_member(int form, const void* in) {
    Fp12<C> a;
    memcpy(&a, in, sizeof(a));
    if (form == 0) return plain_is_member<C>(a) ? 1 : 0;
    if (form == 1) {
      Fp12<C, EH> f;
      load_lp(f, a);
      return gt_is_member_chain<C, GtOpsLp<C, EH>>(f) ? 1 : 0;
    }
    if (form == 2) {
      Fp12Q<C, EQ> f;
      load_q(f, a);
      return gt_is_member_chain<C, GtOpsQ<C, EQ>>(f) ? 1 : 0;
    }
    return -5;
  }
  static int inverse(int form, const void* in, void* out) {
    Fp12<C> a, o;
    memcpy(&a, in, sizeof(a));
    if (form == 0) {
      fp12_inv<C>(o, a);
    } else if (form == 1) {
      Fp12<C, EH> f, r;
      load_lp(f, a);
      GtOpsLp<C, EH>::inv(r, f);
      store_lp(o, r);
    } else if (form == 2) {
      Fp12Q<C, EQ> f, r;
      load_q(f, a);
      GtOpsQ<C, EQ>::inv(r, f);
      store_q(o, r);
    } else {
      return -5;
    }
    memcpy(out, &o, sizeof(o));
    return 0;
  }
};

#define GC_DISPATCH(call)                  \
  switch (curve) {                         \
    case 0: return Gc<Bn254>::call;        \
    case 1: return Gc<Bls381>::call;       \
    case 2: return Gc<Bls377>::call;       \
    default: return -2;                    \
  }

extern "C" {
int gc_is_member(int curve, int form, const void* in) { GC_DISPATCH(is_member(form, in)) }
int gc_inverse(int curve, int form, const void* in, void* out) { GC_DISPATCH(inverse(form, in, out)) }
}
