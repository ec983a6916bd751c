// TEST ARTIFACT -- host (g++) build of pairing_prepared.h, loaded by tests/test_g2_prepared_host.py through ctypes and
// compared with oracle/pyref.py: build lines -> prepared Miller core -> final_exp, over the boundary-form element (the
// one-lane kernel's) and the host models of the carry-free lane pair and quad (every operation checks its weight budget and
// aborts when one is exceeded).  It is NOT part of libmlhip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../mathlib_amd/csrc/pairing_prepared.h"

using namespace mlhip;

template <class C>
struct Prep {
  typedef Affine<FpField<C>> A1;
  typedef Affine<Fp2Field<C>> A2;
  typedef Line<C, Fp2<C>> L32;
  static constexpr int NL = prepared_num_lines<C>();

  // what k_g2_prepare leaves on the device: both images of every line of every Q, and the infinity flags
  struct Tables {
    std::vector<L32> t32;
    std::vector<int32_t> t28;
    std::vector<uint32_t> inf;
  };
  struct Sink {
    L32* l32;
    int32_t* w28;
    int count = 0;
    void operator()(int li, const L32& l) {
      l32[li] = l;
      prepared_line_to28<C>(w28 + (size_t)li * 6 * C::N28, l);
      count++;
    }
  };
  static int build(Tables& t, const A2* Q, int m) {
    t.t32.resize((size_t)m * NL);
    t.t28.resize((size_t)m * prepared_words28<C>());
    t.inf.resize(m);
    for (int i = 0; i < m; i++) {
      t.inf[i] = affine_is_inf<Fp2Field<C>>(Q[i]) ? 1u : 0u;
      Sink s{t.t32.data() + (size_t)i * NL, t.t28.data() + (size_t)i * prepared_words28<C>()};
      g2_prepare_lines<C>(Q[i].x, Q[i].y, s);
      if (s.count != NL) return -3;
    }
    return 0;
  }
  // the carry-free image read the way the kernels' lanes read it: string (coefficient, component) of line li of Q q
  static const int32_t* str28(const Tables& t, uint32_t q, int li, int coef, int comp) {
    return t.t28.data() + ((((size_t)q * NL + li) * 3 + coef) * 2 + comp) * C::N28;
  }
  struct Lines28H {
    const Tables* t;
    uint32_t q[4];
    void load(Line<C, Fp2H28<C>>& l, int k, int li) const {
      Fp2H28<C>* c[3] = {&l.r0, &l.r1, &l.r2};
      for (int j = 0; j < 3; j++) {
        for (int h = 0; h < 2; h++) memcpy(c[j]->c[h].l, str28(*t, q[k], li, j, h), sizeof(int32_t) * C::N28);
        c[j]->wt = 1;
        c[j]->vbound = 1;
      }
    }
  };
  struct Lines28Q {
    const Tables* t;
    uint32_t q[4];
    void load(Line<C, Fp2Q28H<C>>& l, int k, int li) const {
      Fp2Q28H<C>* c[3] = {&l.r0, &l.r1, &l.r2};
      for (int j = 0; j < 3; j++) {
        for (int h = 0; h < 4; h++) memcpy(c[j]->c[h].l, str28(*t, q[k], li, j, h & 1), sizeof(int32_t) * C::N28);
        c[j]->wt = 1;
        c[j]->vbound = 1;
      }
    }
  };

  // form 0: boundary form, 1: lane-pair model, 2: quad model.  out = the product's Miller value (with_fexp: after FExp),
  // canonical.  Returns the largest weight left in the result (1), or a negative error.
  static int run(int form, const void* g1s, const void* g2s, int m, const uint32_t* idx, int ppp, int with_fexp, void* out) {
    const A1* P = (const A1*)g1s;
    Tables t;
    int rc = build(t, (const A2*)g2s, m);
    if (rc) return rc;
    uint32_t q[4] = {0, 0, 0, 0};
    bool live[4] = {false, false, false, false};
    for (int k = 0; k < ppp; k++) {
      q[k] = idx ? idx[k] : (uint32_t)k;
      if (q[k] >= (uint32_t)m) return -4;
      live[k] = !(affine_is_inf<FpField<C>>(P[k]) | (t.inf[q[k]] != 0));
    }
    Fp12<C> o;
    int w = 1;
    if (form == 0) {
      Fp<C> px[4], py[4];
      for (int k = 0; k < ppp; k++) {
        px[k] = P[k].x;
        py[k] = P[k].y;
      }
      PreparedLines32<C> ls;
      ls.tab = t.t32.data();
      memcpy(ls.q, q, sizeof(q));
      Fp12<C> f, r;
      miller_loop_prepared_core<C, 4, Fp2<C>, Fp<C>>(f, px, py, live, ppp, ls);
      if (with_fexp) {
        final_exp<C>(r, f);
        f = r;
      }
      o = f;
    } else {
      Fp28<C> px[4], py[4];
      for (int k = 0; k < ppp; k++) {
        fp28_from_fp<C>(px[k], P[k].x);
        fp28_from_fp<C>(py[k], P[k].y);
      }
      if (form == 1) {
        typedef Fp2H28<C> E;
        Lines28H ls{&t, {q[0], q[1], q[2], q[3]}};
        Fp12<C, E> f, r;
        miller_loop_prepared_core<C, 4, E, Fp28<C>>(f, px, py, live, ppp, ls);
        if (with_fexp) {
          final_exp<C>(r, f);
          f = r;
        }
        Fp2<C>* d = &o.c0.c0;
        const E* s = &f.c0.c0;
        for (int i = 0; i < 6; i++) {
          fp28_to_fp<C>(d[i].c0, s[i].c[0]);
          fp28_to_fp<C>(d[i].c1, s[i].c[1]);
          w = s[i].wt > w ? s[i].wt : w;
        }
      } else if (form == 2) {
        typedef Fp2Q28H<C> E;
        Lines28Q ls{&t, {q[0], q[1], q[2], q[3]}};
        Fp12Q<C, E> f, r;
        miller_loop_prepared_q<C, 4, E, Fp28<C>>(f, px, py, live, ppp, ls);
        if (with_fexp) {
          final_exp_q<C>(r, f);
          f = r;
        }
        Fp2<C>* lo = &o.c0.c0;
        Fp2<C>* up = &o.c1.c0;
        const E* s = &f.v.c0;
        for (int j = 0; j < 3; j++) {
          fp28_to_fp<C>(lo[j].c0, s[j].c[0]);
          fp28_to_fp<C>(lo[j].c1, s[j].c[1]);
          fp28_to_fp<C>(up[j].c0, s[j].c[2]);
          fp28_to_fp<C>(up[j].c1, s[j].c[3]);
          w = s[j].wt > w ? s[j].wt : w;
        }
      } else {
        return -5;
      }
    }
    memcpy(out, &o, sizeof(o));
    return w;
  }

  // the general loop (pairing.h: miller_loop_core over the boundary form) on explicit pairs, for the comparison
  static int general(const void* g1s, const void* g2s, int ppp, int with_fexp, void* out) {
    Fp12<C> f, r;
    miller_loop<C, 4>(f, (const A1*)g1s, (const A2*)g2s, ppp);
    if (with_fexp) {
      final_exp<C>(r, f);
      f = r;
    }
    memcpy(out, &f, sizeof(f));
    return 1;
  }
};

extern "C" {
int hp_num_lines(int curve) {
  switch (curve) {
    case 0: return Prep<Bn254>::NL;
    case 1: return Prep<Bls381>::NL;
    case 2: return Prep<Bls377>::NL;
    default: return -2;
  }
}
int hp_prepared(int curve, int form, const void* g1s, const void* g2s, int m, const uint32_t* idx, int ppp, int with_fexp,
                void* out) {
  switch (curve) {
    case 0: return Prep<Bn254>::run(form, g1s, g2s, m, idx, ppp, with_fexp, out);
    case 1: return Prep<Bls381>::run(form, g1s, g2s, m, idx, ppp, with_fexp, out);
    case 2: return Prep<Bls377>::run(form, g1s, g2s, m, idx, ppp, with_fexp, out);
    default: return -2;
  }
}
int hp_general(int curve, const void* g1s, const void* g2s, int ppp, int with_fexp, void* out) {
  switch (curve) {
    case 0: return Prep<Bn254>::general(g1s, g2s, ppp, with_fexp, out);
    case 1: return Prep<Bls381>::general(g1s, g2s, ppp, with_fexp, out);
    case 2: return Prep<Bls377>::general(g1s, g2s, ppp, with_fexp, out);
    default: return -2;
  }
}
}
