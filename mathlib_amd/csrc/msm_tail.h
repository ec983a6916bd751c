// msm_tail.h -- the tail of an MSM as a kernel, for device-result plans (include/mlhip.h, "device results"; DESIGN.md
// section 16): what msm_plan.h's host_tail / host_tail_fold compute on the host from the W x nsel partial sums the
// reduction leaves in d_out -- the per-window sums (host_tail_window's loop), the Horner pass over the plan's window
// layout (horner_jac's pass) and the conversion to an affine point -- written into a slot the plan owns, in stream order.
//
// The arithmetic is in MLHIP_HD bodies over a lane policy P, so that a g++ build replays it job by job
// (tests/hostmath_tail):
//   P::FW    the field the arithmetic runs on: F itself with one lane per window (G1; and the host replay of both groups),
//            Fp2LField<C> with one lane PAIR per window (G2 on the device: one Fp2 component per lane, fp2_lanes.h)
//   P::Mem / P::AffMem    XYZZ<F> / Affine<F>: what memory holds (d_out, the LDS array of window sums, the result slot)
//   P::load / P::store / P::store_affine    between the two
// Two phases, as on the host: msm_tail_window is job w of host_parallel (independent chains of nb + lgL doublings and
// nb + 4 additions), msm_tail_total the sequential rest.  Every addition is a complete one (ec.h: xyzz_add, ec_jac.h:
// jac_add -- infinity on either side, equal and opposite operands): an empty window, a window sum that equals the running
// Horner value or cancels it are ordinary inputs here.
#pragma once
#include "ec_jac.h"
#include "msm_body.h"

namespace mlhip {

constexpr int MSM_TAIL_MAX_W = 64;  // windows of a plan: ceil((bits + 1) / c) with bits <= 255 and c >= 4

// What the kernel needs of a plan, by value (msm_plan.h: msm_tail_args fills it).
//   plain plan:   W window sums over out[w nsel ..], then the Horner pass with down[] (msm_window_shifts of the plan's OWN
//                 scalar width: a short-scalar plan has its shorter layout)
//   folded plan:  ONE "window" -- the fold_nsel2 combined entries behind the W x nsel ones (first = W nsel, nb =
//                 fold_nsel2 - 4), or, where the plan has a single bucket group, that group's nsel entries (first = 0) --
//                 and no Horner pass (host_tail_fold: the lg M doublings apply to an empty sum there)
struct MsmTailArgs {
  int W;       // window sums to form
  int nsel;    // entries between two windows' partial sums
  int nb;      // bit-masked sums per window: entries 4 .. 4 + nb - 1
  int lgL;     // their common weight 2^lgL
  int first;   // entry the first window starts at
  int horner;  // 1: the Horner pass over the W sums; 0: the total is the single sum
  int empty;   // 1: an MSM of no pairs -- nothing is read, the result is the point at infinity
  unsigned char down[MSM_TAIL_MAX_W];  // doublings after adding window w (down[0] = 0; at most c + 1 <= 21 each)
};

// one lane per window: memory and registers hold the same type
template <class F>
struct TailOneLane {
  typedef F FW;
  typedef XYZZ<F> Mem;
  typedef Affine<F> AffMem;
  MLHIP_HD static void load(XYZZ<F>& r, const Mem* src, size_t i) { r = src[i]; }
  MLHIP_HD static void store(Mem* dst, size_t i, const XYZZ<F>& r) { dst[i] = r; }
  MLHIP_HD static void store_affine(AffMem* dst, const Affine<F>& r) { *dst = r; }
};

// V[w] = out[0..3] summed + 2^lgL sum_k 2^k out[4 + k] of window w: host_tail_window's loop, operation for operation
template <class P>
MLHIP_HD void msm_tail_window(const MsmTailArgs& a, int w, const typename P::Mem* out, typename P::Mem* V) {
  typedef typename P::FW FW;
  const size_t o = (size_t)a.first + (size_t)w * a.nsel;
  XYZZ<FW> acc, d, q;
  xyzz_set_inf<FW>(acc);
  for (int k = a.nb - 1; k >= 0; k--) {
    xyzz_dbl<FW>(d, acc);
    acc = d;
    P::load(q, out, o + 4 + k);
    xyzz_add<FW>(acc, q);
  }
  for (int k = 0; k < a.lgL; k++) {
    xyzz_dbl<FW>(d, acc);
    acc = d;
  }
  for (int k = 0; k < 4; k++) {
    P::load(q, out, o + k);
    xyzz_add<FW>(acc, q);
  }
  P::store(V, w, acc);
}

// the sequential rest: total = sum_w 2^off(w) V[w] by horner_jac's pass (Jacobian doublings, one per scalar bit), or the
// single sum of a folded plan; then the affine point.  Writes the XYZZ value and the affine point.
template <class P>
MLHIP_HD void msm_tail_total(const MsmTailArgs& a, const typename P::Mem* V, typename P::Mem* res_xyzz,
                             typename P::AffMem* res_affine) {
  typedef typename P::FW FW;
  XYZZ<FW> total;
  if (a.empty) {
    xyzz_set_inf<FW>(total);
  } else if (!a.horner) {
    P::load(total, V, 0);
  } else {
    Jac<FW> acc, v;
    XYZZ<FW> x;
    jac_set_inf<FW>(acc);
    for (int i = 0; i < a.W; i++) {
      const int w = a.W - 1 - i;
      P::load(x, V, w);
      jac_from_xyzz<FW>(v, x);
      jac_add<FW>(acc, v);
      const int dn = a.down[w];
      for (int k = 0; k < dn; k++) jac_dbl<FW>(acc, acc);
    }
    jac_to_xyzz<FW>(total, acc);
  }
  Affine<FW> r;
  xyzz_to_affine<FW>(r, total);
  P::store(res_xyzz, 0, total);
  P::store_affine(res_affine, r);
}

#if defined(__HIPCC__)
// ---- the kernel (gfx950) ------------------------------------------------------------------------------------------------
// G2: one lane pair per window, on Fp2LField<C> with the component loads of msm_g2.h (as k_scalar_mul_lp).  Every branch of
// the bodies above is taken on values both lanes of a pair hold (fp2_is_zero exchanges its verdict), so a pair stays in one
// control flow.
template <class C>
struct TailLanePair {
  typedef Fp2LField<C> FW;
  typedef XYZZ<Fp2Field<C>> Mem;
  typedef Affine<Fp2Field<C>> AffMem;
  __device__ static void load(XYZZ<FW>& r, const Mem* src, size_t i) { lp_load_xyzz<C>(r, src, i, (int)(threadIdx.x & 1u)); }
  __device__ static void store(Mem* dst, size_t i, const XYZZ<FW>& r) { lp_store_xyzz<C>(dst, i, r, (int)(threadIdx.x & 1u)); }
  __device__ static void store_affine(AffMem* dst, const Affine<FW>& r) {
    const int hi = (int)(threadIdx.x & 1u);
    Fp<C>* o = reinterpret_cast<Fp<C>*>(dst);
    o[hi] = r.x.v;
    o[2 + hi] = r.y.v;
  }
};

// One workgroup of 64 LANES lanes: lane (pair) w < W forms V[w] in LDS (64 x 192 B for G1, 64 x 384 B for G2 on the 12-limb
// fields), every lane reaches the barrier -- lanes beyond W skip the arithmetic, not the barrier -- and lane (pair) 0 runs
// the rest.  Bound by the latency of one lane's chain of doublings (one per scalar bit); nothing here is tuned for speed.
template <class P, int LANES>
__global__ void __launch_bounds__(64 * LANES) k_msm_tail(const typename P::Mem* __restrict__ out, const MsmTailArgs a,
                                                         typename P::Mem* __restrict__ res_xyzz,
                                                         typename P::AffMem* __restrict__ res_affine) {
  typedef typename P::Mem Mem;
  __shared__ __attribute__((aligned(16))) unsigned char raw[MSM_TAIL_MAX_W * sizeof(Mem)];
  Mem* V = reinterpret_cast<Mem*>(raw);
  const int w = (int)threadIdx.x / LANES;
  if (!a.empty && w < a.W) msm_tail_window<P>(a, w, out, V);
  __syncthreads();
  if ((int)threadIdx.x < LANES) msm_tail_total<P>(a, V, res_xyzz, res_affine);
}
#endif

}  // namespace mlhip
