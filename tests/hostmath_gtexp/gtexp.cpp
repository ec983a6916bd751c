// TEST ARTIFACT -- host (g++) build of gt_exp_cyclo.h and of pairing_quad.h's fp12q_cyclo_sqr, loaded by
// tests/test_gt_exp_cyclo_host.py through ctypes and compared with Python integers and oracle/pyref.py: the scalar split, the
// quad Granger-Scott squaring against the generic quad squaring, and the whole chain through the host models of the
// carry-free lane pair and quad (every operation checks its weight and value budget and aborts when one is exceeded); the
// 4-bit windowed chain of mlhip_gt_exp through the same two models and over the plain tower (tower.h on Fp2<C>).
// It is NOT part of libmlhip.so.
#include <stdint.h>
#include <string.h>
#include "../../mathlib_amd/csrc/gt_exp_cyclo.h"

using namespace mlhip;

template <class C>
struct Gx {
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
  static int store_lp(Fp12<C>& out, const Fp12<C, EH>& f) {
    Fp2<C>* d = &out.c0.c0;
    const EH* s = &f.c0.c0;
    int w = 1;
    for (int i = 0; i < 6; i++) {
      fp28_to_fp<C>(d[i].c0, s[i].c[0]);
      fp28_to_fp<C>(d[i].c1, s[i].c[1]);
      w = s[i].wt > w ? s[i].wt : w;
    }
    return w;
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
  static int store_q(Fp12<C>& out, const Fp12Q<C, EQ>& f) {
    Fp2<C>* lo = &out.c0.c0;
    Fp2<C>* up = &out.c1.c0;
    const EQ* s = &f.v.c0;
    int w = 1;
    for (int j = 0; j < 3; j++) {
      fp28_to_fp<C>(lo[j].c0, s[j].c[0]);
      fp28_to_fp<C>(lo[j].c1, s[j].c[1]);
      fp28_to_fp<C>(up[j].c0, s[j].c[2]);
      fp28_to_fp<C>(up[j].c1, s[j].c[3]);
      w = s[j].wt > w ? s[j].wt : w;
    }
    return w;
  }

  // dig = the digits of the canonical scalar behind `scalar` (fr_canonical first, as the kernels; mont < 0: the split of
  // the 256-bit value as it is)
  static int split(const uint32_t* scalar, int mont, uint32_t* dig_out, uint32_t* canon_out) {
    uint32_t s[8], dig[8];
    if (mont < 0)
      memcpy(s, scalar, sizeof(s));
    else
      fr_canonical<C>(s, scalar, mont != 0);
    gt_exp_split<C>(dig, s);
    memcpy(dig_out, dig, sizeof(dig));
    memcpy(canon_out, s, sizeof(s));
    return GtSplit<C>::DIM;
  }

  // the quad Granger-Scott squaring and the generic quad squaring of one value; returns the largest weight left
  static int cyclo_sqr(const void* in, void* out_cyclo, void* out_generic) {
    Fp12<C> a, o;
    memcpy(&a, in, sizeof(a));
    Fp12Q<C, EQ> f, r;
    load_q(f, a);
    fp12q_cyclo_sqr<C>(r, f);
    int w = store_q(o, r);
    memcpy(out_cyclo, &o, sizeof(o));
    fp12q_sqr<C>(r, f);
    int w2 = store_q(o, r);
    memcpy(out_generic, &o, sizeof(o));
    return w > w2 ? w : w2;
  }

  // form 1: lane-pair model, 2: quad model; out = in^scalar by the chain of the kernels
  static int exp(int form, const void* in, const uint32_t* scalar, int mont, void* out) {
    Fp12<C> a, o;
    memcpy(&a, in, sizeof(a));
    uint32_t s[8], dig[8];
    fr_canonical<C>(s, scalar, mont != 0);
    gt_exp_split<C>(dig, s);
    int w;
    if (form == 1) {
      static Fp12<C, EH> tab[15];
      Fp12<C, EH> acc;
      load_lp(tab[0], a);
      gt_exp_cyclo_chain<C, GtOpsLp<C, EH>>(acc, tab, dig);
      w = store_lp(o, acc);
    } else if (form == 2) {
      static Fp12Q<C, EQ> tab[15];
      Fp12Q<C, EQ> acc;
      load_q(tab[0], a);
      gt_exp_cyclo_chain<C, GtOpsQ<C, EQ>>(acc, tab, dig);
      w = store_q(o, acc);
    } else {
      return -5;
    }
    memcpy(out, &o, sizeof(o));
    return w;
  }

  // the same for the windowed chain, valid for any Fp12 value; form 0: the plain tower (the shape of the saturated kernel)
  static int exp_window(int form, const void* in, const uint32_t* scalar, int mont, void* out) {
    Fp12<C> a, o;
    memcpy(&a, in, sizeof(a));
    uint32_t s[8];
    fr_canonical<C>(s, scalar, mont != 0);
    int w = 1;
    if (form == 0) {
      static Fp12<C> tab[15];
      tab[0] = a;
      gt_exp_window_chain<C, GtOpsLp<C, Fp2<C>>>(o, tab, s);
    } else if (form == 1) {
      static Fp12<C, EH> tab[15];
      Fp12<C, EH> acc;
      load_lp(tab[0], a);
      gt_exp_window_chain<C, GtOpsLp<C, EH>>(acc, tab, s);
      w = store_lp(o, acc);
    } else if (form == 2) {
      static Fp12Q<C, EQ> tab[15];
      Fp12Q<C, EQ> acc;
      load_q(tab[0], a);
      gt_exp_window_chain<C, GtOpsQ<C, EQ>>(acc, tab, s);
      w = store_q(o, acc);
    } else {
      return -5;
    }
    memcpy(out, &o, sizeof(o));
    return w;
  }
};

#define GX_DISPATCH(call)                  \
  switch (curve) {                         \
    case 0: return Gx<Bn254>::call;        \
    case 1: return Gx<Bls381>::call;       \
    case 2: return Gx<Bls377>::call;       \
    default: return -2;                    \
  }

extern "C" {
// the modulus of the split (two 64-bit halves) and the number of digits
int gx_modulus(int curve, uint64_t* lo, uint64_t* hi) {
  switch (curve) {
    case 0: *lo = GtSplit<Bn254>::LO; *hi = GtSplit<Bn254>::HI; return GtSplit<Bn254>::DIM;
    case 1: *lo = GtSplit<Bls381>::LO; *hi = GtSplit<Bls381>::HI; return GtSplit<Bls381>::DIM;
    case 2: *lo = GtSplit<Bls377>::LO; *hi = GtSplit<Bls377>::HI; return GtSplit<Bls377>::DIM;
    default: return -2;
  }
}
int gx_split(int curve, const uint32_t* scalar, int mont, uint32_t* dig, uint32_t* canon) { GX_DISPATCH(split(scalar, mont, dig, canon)) }
int gx_cyclo_sqr(int curve, const void* in, void* out_cyclo, void* out_generic) { GX_DISPATCH(cyclo_sqr(in, out_cyclo, out_generic)) }
int gx_exp(int curve, int form, const void* in, const uint32_t* scalar, int mont, void* out) { GX_DISPATCH(exp(form, in, scalar, mont, out)) }
int gx_exp_window(int curve, int form, const void* in, const uint32_t* scalar, int mont, void* out) { GX_DISPATCH(exp_window(form, in, scalar, mont, out)) }
}
