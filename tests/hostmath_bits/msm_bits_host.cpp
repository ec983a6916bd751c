// tests/hostmath_bits -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of what a short-scalar MSM
// plan (mlhip_msm_plan_create_bits) adds to the headers: the width rule (msm_effective_c), the layout over bits + 1 bits,
// the masked canonical scalar (fr_canonical_bits), the digits (msm_digits_body with the plan's width) and a whole G1 MSM
// replayed in the kernels' order -- digits, buckets, per-window sums, then the host tail's Horner pass over the short
// layout (msm_window_shifts + horner_jac, as msm_plan.h: host_tail runs them).  Driven by tests/test_msm_bits_host.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_body.h"
#include "../../mathlib_amd/csrc/ec_jac.h"

using namespace mlhip;

template <class C>
struct Bits {
  typedef FpField<C> F;
  typedef Affine<F> A;
  typedef XYZZ<F> X;

  static int digits(const void* scalar, int mont, int c, int bits, uint32_t* out, int cap) {
    const int W = msm_num_windows(bits, c);
    if (W > cap) return -3;
    msm_digits_body<C>(0, 1, (const uint32_t*)scalar, mont != 0, c, W, out, bits);
    return W;
  }
  static int masked(const void* scalar, int mont, int bits, void* out) {
    uint32_t s[8];
    fr_canonical_bits<C>(s, (const uint32_t*)scalar, mont != 0, bits);
    memcpy(out, s, 32);
    return 0;
  }
  // sum_i [(s_i mod r) mod 2^bits] P_i with the plan's width c (already the effective one) -- one thread's worth of every
  // kernel in turn: the digit rows [W][n], one XYZZ bucket per (window, magnitude), the window sums V_w = sum_b (b + 1) B_b
  // by the running-sum rule, and the Horner pass of the host tail
  static int msm(const void* points, const void* scalars, int mont, size_t n, int c, int bits, void* out) {
    const int W = msm_num_windows(bits, c);
    const size_t M = (size_t)1 << (c - 1);
    const A* pts = (const A*)points;
    std::vector<uint32_t> dig((size_t)W * n);
    for (size_t i = 0; i < n; i++) msm_digits_body<C>(i, n, (const uint32_t*)scalars, mont != 0, c, W, dig.data(), bits);
    std::vector<X> buckets((size_t)W * M);
    for (X& b : buckets) xyzz_set_inf<F>(b);
    for (int w = 0; w < W; w++)
      for (size_t i = 0; i < n; i++) {
        const uint32_t d = dig[(size_t)w * n + i];
        if (!d) continue;
        const size_t mag = d >> 1;
        if (mag > M) return -4;  // a digit above its window: the mask or the layout is wrong
        xyzz_madd<F>(buckets[(size_t)w * M + mag - 1], pts[i], (d & 1u) != 0);
      }
    std::vector<X> V(W);
    for (int w = 0; w < W; w++) {
      X run, tot;
      xyzz_set_inf<F>(run);
      xyzz_set_inf<F>(tot);
      for (size_t b = M; b-- > 0;) {
        xyzz_add<F>(run, buckets[(size_t)w * M + b]);
        xyzz_add<F>(tot, run);
      }
      V[w] = tot;
    }
    std::vector<int> down(W, 0);
    msm_window_shifts(bits, c, down.data());
    X total;
    horner_jac<F>(total, V.data(), W, down.data());
    A r;
    xyzz_to_affine<F>(r, total);
    memcpy(out, &r, sizeof(A));
    return W;
  }
};

#define DISPATCH(curve, call)                \
  switch (curve) {                           \
    case 0: return Bits<Bn254>::call;        \
    case 1: return Bits<Bls381>::call;       \
    case 2: return Bits<Bls377>::call;       \
    default: return -1;                      \
  }

extern "C" {
int mb_effective_c(int bits, int c) { return msm_effective_c(bits, c); }
// out = {W, base, rem} of the balanced layout over bits + 1 bits at width c
int mb_layout(int bits, int c, int* out) {
  const WinLayout l = msm_win_layout(bits, c);
  out[0] = l.W;
  out[1] = l.base;
  out[2] = l.rem;
  return 0;
}
// out[w] = doublings between windows w and w - 1 in the host tail; returns W
int mb_shifts(int bits, int c, int* out, int cap) {
  const int W = msm_num_windows(bits, c);
  if (W > cap) return -3;
  msm_window_shifts(bits, c, out);
  return W;
}
int mb_fr_bits(int curve) {
  switch (curve) {
    case 0: return Bn254::FR_BITS;
    case 1: return Bls381::FR_BITS;
    case 2: return Bls377::FR_BITS;
    default: return -1;
  }
}
int mb_digits(int curve, const void* scalar, int mont, int c, int bits, uint32_t* out, int cap) {
  DISPATCH(curve, digits(scalar, mont, c, bits, out, cap))
}
int mb_masked(int curve, const void* scalar, int mont, int bits, void* out) { DISPATCH(curve, masked(scalar, mont, bits, out)) }
int mb_msm(int curve, const void* points, const void* scalars, int mont, size_t n, int c, int bits, void* out) {
  DISPATCH(curve, msm(points, scalars, mont, n, c, bits, out))
}
}
