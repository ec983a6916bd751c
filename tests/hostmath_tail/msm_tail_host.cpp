// tests/hostmath_tail -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the tail kernel's bodies
// (mathlib_amd/csrc/msm_tail.h: msm_tail_window, msm_tail_total over the one-lane policy), replayed job by job as
// k_msm_tail runs them, beside what a host-result plan computes from the same partial sums: host_tail_window per window,
// horner_jac over msm_window_shifts, xyzz_to_affine (msm_plan.h: host_tail, host_tail_fold).  G1 and G2 of the three curves.
// Driven by tests/test_msm_tail_host.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/mlhip.h"
#include "../../mathlib_amd/csrc/msm_tail.h"

using namespace mlhip;

template <class F>
struct Tail {
  typedef Affine<F> A;
  typedef XYZZ<F> X;
  typedef TailOneLane<F> P;

  // (X l^2, Y l^3, l^2, l^3) for the affine point (X, Y) and a field element l: the same point, another representative
  static int scaled(const void* affine, const void* lambda, void* out) {
    A p;
    typename F::T l, l2, l3;
    memcpy(&p, affine, sizeof(A));
    memcpy(&l, lambda, sizeof(l));
    X r;
    if (affine_is_inf<F>(p) || F::is_zero(l)) {
      xyzz_set_inf<F>(r);
    } else {
      F::sqr(l2, l);
      F::mul(l3, l2, l);
      F::mul(r.x, p.x, l2);
      F::mul(r.y, p.y, l3);
      r.zz = l2;
      r.zzz = l3;
    }
    memcpy(out, &r, sizeof(X));
    return 0;
  }
  static int to_affine(const void* xyzz, void* out) {
    X x;
    A r;
    memcpy(&x, xyzz, sizeof(X));
    xyzz_to_affine<F>(r, x);
    memcpy(out, &r, sizeof(A));
    return xyzz_is_inf<F>(x) ? 1 : 0;
  }
  // the kernel: phase 1 for every lane w < W, the barrier, phase 2 on lane 0
  static int kernel(const MsmTailArgs& a, const void* entries, void* res_xyzz, void* res_affine) {
    if (a.W > MSM_TAIL_MAX_W) return -3;
    std::vector<X> V(MSM_TAIL_MAX_W);
    for (int lane = 0; lane < 64; lane++)
      if (!a.empty && lane < a.W) msm_tail_window<P>(a, lane, (const X*)entries, V.data());
    msm_tail_total<P>(a, V.data(), (X*)res_xyzz, (A*)res_affine);
    return 0;
  }
  // the host tail: a blob {header, entries from `first`} per host_tail / host_tail_fold, host_tail_window per window, then
  // horner_jac with the layout's shifts (plain plan) or the single window's sum (folded plan)
  static int host(const MsmTailArgs& a, const void* entries, int bits, int c, void* res_xyzz, void* res_affine) {
    // (the combined entries of a folded plan: one window of 4 + nb entries, more than the nsel of its groups)
    const size_t count = (size_t)(a.W - 1) * a.nsel + (size_t)(a.nsel > 4 + a.nb ? a.nsel : 4 + a.nb);
    std::vector<unsigned char> blob(sizeof(HostTailHeader) + count * sizeof(X));
    const HostTailHeader h{a.nb, a.lgL, a.nsel, 0};
    memcpy(blob.data(), &h, sizeof(h));
    memcpy(blob.data() + sizeof(h), (const X*)entries + a.first, count * sizeof(X));
    std::vector<X> V(a.W);
    for (int w = 0; w < a.W; w++) host_tail_window<F>(blob.data(), w, &V[w]);
    X total;
    if (a.empty) {
      xyzz_set_inf<F>(total);
    } else if (a.horner) {
      std::vector<int> down(a.W, 0);
      msm_window_shifts(bits, c, down.data());
      horner_jac<F>(total, V.data(), a.W, down.data());
    } else {
      total = V[0];
    }
    A r;
    xyzz_to_affine<F>(r, total);
    memcpy(res_xyzz, &total, sizeof(X));
    memcpy(res_affine, &r, sizeof(A));
    return 0;
  }
};

#define DISPATCH(curve, group, call)                                             \
  switch ((curve) * 2 + ((group) == 2 ? 1 : 0)) {                                \
    case 0: return Tail<FpField<Bn254>>::call;                                   \
    case 1: return Tail<Fp2Field<Bn254>>::call;                                  \
    case 2: return Tail<FpField<Bls381>>::call;                                  \
    case 3: return Tail<Fp2Field<Bls381>>::call;                                 \
    case 4: return Tail<FpField<Bls377>>::call;                                  \
    case 5: return Tail<Fp2Field<Bls377>>::call;                                 \
    default: return -1;                                                          \
  }

static MsmTailArgs make_args(int W, int nsel, int nb, int lgL, int first, int horner, int empty, const int* down) {
  MsmTailArgs a;
  memset(&a, 0, sizeof(a));
  a.W = W;
  a.nsel = nsel;
  a.nb = nb;
  a.lgL = lgL;
  a.first = first;
  a.horner = horner;
  a.empty = empty;
  for (int w = 0; w < W && w < MSM_TAIL_MAX_W; w++) a.down[w] = (unsigned char)(down ? down[w] : 0);
  return a;
}

extern "C" {
int mt_max_windows(void) { return MSM_TAIL_MAX_W; }
int mt_flag(void) { return MLHIP_WINDOW_DEVICE_RESULT; }
int mt_window_bits(int c, int bits) { return MLHIP_WINDOW_BITS(c, bits); }
int mt_num_windows(int bits, int c) { return msm_num_windows(bits, c); }
// out[w] = doublings after window w in the Horner pass of a plan over `bits`-bit scalars at width c; returns W
int mt_shifts(int bits, int c, int* out, int cap) {
  const int W = msm_num_windows(bits, c);
  if (W > cap) return -3;
  msm_window_shifts(bits, c, out);
  return W;
}
int mt_scaled(int curve, int group, const void* affine, const void* lambda, void* out) {
  DISPATCH(curve, group, scaled(affine, lambda, out))
}
int mt_to_affine(int curve, int group, const void* xyzz, void* out) { DISPATCH(curve, group, to_affine(xyzz, out)) }
// the kernel's replay: `down` as the plan hands it over (msm_plan.h: msm_tail_args)
int mt_kernel(int curve, int group, const void* entries, int W, int nsel, int nb, int lgL, int first, int horner, int empty,
              const int* down, void* res_xyzz, void* res_affine) {
  const MsmTailArgs a = make_args(W, nsel, nb, lgL, first, horner, empty, down);
  DISPATCH(curve, group, kernel(a, entries, res_xyzz, res_affine))
}
// the host-result plan's tail on the same entries; the shifts come from (bits, c) as host_tail takes them
int mt_host(int curve, int group, const void* entries, int W, int nsel, int nb, int lgL, int first, int horner, int empty,
            int bits, int c, void* res_xyzz, void* res_affine) {
  const MsmTailArgs a = make_args(W, nsel, nb, lgL, first, horner, empty, nullptr);
  DISPATCH(curve, group, host(a, entries, bits, c, res_xyzz, res_affine))
}
}
