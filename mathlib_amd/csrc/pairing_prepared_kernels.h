// pairing_prepared_kernels.h -- the kernels behind mlhip_g2_prepared_* (include/mlhip.h): building a handle's line tables
// and the Miller loops / fused pairings that read them (pairing_prepared.h).  Included by tu_pairing_<curve>.hip (one code object per curve).
// Replaces, for fixed G2 arguments, MillerLoop + FinalExponentiation behind the reference's Pairing, Pairing2 and FExp
// (driver/gurvy/bls12381/bls12-381.go:448-468, bn254.go:247-267, bls12-377.go:244-264).
#pragma once
#include "pairing_kernels.h"
#include "pairing_prepared.h"

namespace mlhip {

// what the consuming kernels get by value: the tables of a handle and the Q of each slot of a product
template <class C>
struct PreparedView {
  const int32_t* t28;          // [m][NL][r0 r1 r2][c0 c1][N28]
  const Line<C, Fp2<C>>* t32;  // [m][NL]; test build only (nullptr in the product)
  const uint32_t* q_inf;       // [m]: 1 = this Q is the point at infinity
  uint32_t q[4];               // the Q of each slot of a product of at most 4 pairs ...
  const uint32_t* d_index;     // ... or, for longer products, the Q of every slot: a device copy of q_index (else nullptr)
  // the Q of pair k of the group whose first pair sits in slot `slot` of its product (pairing_products.h)
  __device__ __forceinline__ uint32_t q_of(uint32_t slot, int k) const { return d_index ? d_index[slot + k] : q[k]; }
};

// ---- build: one Q per lane, boundary-form arithmetic (runs once per handle) -------------------------------------------
template <class C>
struct PreparedSink {
  int32_t* w28;
  Line<C, Fp2<C>>* l32;
  __device__ void operator()(int li, const Line<C, Fp2<C>>& l) {
    if (l32) l32[li] = l;
    prepared_line_to28<C>(w28 + (size_t)li * 6 * C::N28, l);
  }
};
template <class C>
__global__ void __launch_bounds__(64) k_g2_prepare(const Affine<Fp2Field<C>>* __restrict__ q, size_t m,
                                                   int32_t* __restrict__ t28, Line<C, Fp2<C>>* __restrict__ t32,
                                                   uint32_t* __restrict__ q_inf) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Affine<Fp2Field<C>> Q = q[i];
  q_inf[i] = affine_is_inf<Fp2Field<C>>(Q) ? 1u : 0u;
  PreparedSink<C> sink{t28 + i * prepared_words28<C>(), t32 ? t32 + i * prepared_num_lines<C>() : nullptr};
  g2_prepare_lines<C>(Q.x, Q.y, sink);
}

// out[i * ppp + j] = q[idx[j]]: the G2 array the general kernels want (the dispatcher's fallback)
template <class C>
__global__ void __launch_bounds__(256) k_g2_prepared_expand(const Affine<Fp2Field<C>>* __restrict__ q, PreparedView<C> pv,
                                                            int ppp, size_t n, Affine<Fp2Field<C>>* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * (size_t)ppp) return;
  out[t] = q[pv.q[t % (size_t)ppp]];
}

// ---- one lane per product over Fp2<C> / Fp<C>: the reference shape (test build, MLHIP_PAIRING_ONE_LANE=1) ----------------
// WHAT: 0 = Miller loop, 2 = Miller loop + final exponentiation
template <class C, int WHAT>
__global__ void __launch_bounds__(64) k_miller_prepared(PreparedView<C> pv, const Affine<FpField<C>>* __restrict__ g1,
                                                        MillerGroups mg, size_t n, Fp12<C>* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MillerGroupAt at(mg, i);
  const int ppp = at.count;
  Fp<C> px[4], py[4];
  bool live[4];
  PreparedLines32<C> ls;
  ls.tab = pv.t32;
  for (int k = 0; k < 4; k++) ls.q[k] = k < ppp ? pv.q_of(at.slot, k) : 0u;
  for (int k = 0; k < ppp && k < 4; k++) {
    const Affine<FpField<C>> P = g1[at.first + k];
    px[k] = P.x;
    py[k] = P.y;
    live[k] = !(affine_is_inf<FpField<C>>(P) | (pv.q_inf[ls.q[k]] != 0));
  }
  Fp12<C> f, r;
  miller_loop_prepared_core<C, 4, Fp2<C>, Fp<C>>(f, px, py, live, ppp, ls);
  if (WHAT == 0) {
    out[i] = f;
  } else {
    final_exp<C>(r, f);
    out[i] = r;
  }
}

// ---- carry-free lane pairs / quads: a lane reads the N28-limb strings of ITS Fp2 component -----------------------------------
// The address depends on the slot, the line and the lane's parity only: every lane pair (quad) of a wave reads the same two
// strings, so a wave's load instruction touches two runs of 4 N28 bytes -- one or two cache lines, served by the vector L1
// after the first wave of a CU has pulled them in (a Q's table is 23 KB on BLS12-381).
template <class C>
struct PreparedLines28 {
  const int32_t* tab;
  uint32_t q[4];
  int hi;
  __device__ __forceinline__ void load(Line<C, Fp2L28<C>>& l, int k, int li) const {
    static_assert(C::N28 % 2 == 0, "the strings are read as 8-byte words");
    const int2* p = reinterpret_cast<const int2*>(tab + (((size_t)q[k] * prepared_num_lines<C>() + li) * 6 + hi) * C::N28);
#pragma unroll
    for (int i = 0; i < C::N28 / 2; i++) {
      const int2 a = p[i], b = p[C::N28 + i], c = p[2 * C::N28 + i];  // r1 / r2 lie 2 N28 words = N28 int2 further each
      l.r0.v.l[2 * i] = a.x;
      l.r0.v.l[2 * i + 1] = a.y;
      l.r1.v.l[2 * i] = b.x;
      l.r1.v.l[2 * i + 1] = b.y;
      l.r2.v.l[2 * i] = c.x;
      l.r2.v.l[2 * i + 1] = c.y;
    }
  }
};

// (q: the Q of each pair of this group, PreparedLines28::q)
template <class C, int MAXP>
__device__ __forceinline__ void prepared_load_g1(Fp28<C>* px, Fp28<C>* py, bool* live, const PreparedView<C>& pv,
                                                 const Affine<FpField<C>>* __restrict__ g1, size_t first, int ppp,
                                                 const uint32_t* q) {
  for (int k = 0; k < ppp && k < MAXP; k++) {
    const Affine<FpField<C>> P = g1[first + k];
    live[k] = !(affine_is_inf<FpField<C>>(P) | (pv.q_inf[q[k]] != 0));
    fp28_from_fp<C>(px[k], P.x);
    fp28_from_fp<C>(py[k], P.y);
  }
}

// two lanes per product.  WHAT: 0 = Miller loop, 2 = Miller loop + final exponentiation; MAXP: 1 for ppp = 1 (the per-pair
// arrays are then registers), 4 otherwise -- the conventions of k_pairing_lp28
template <class C, int WHAT, int MAXP>
__global__ void __launch_bounds__(64) MLHIP_LP_OCC k_pairing_prep_lp28(PreparedView<C> pv,
                                                                       const Affine<FpField<C>>* __restrict__ g1,
                                                                       MillerGroups mg, size_t n, Fp12<C>* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 1;  // both lanes of a pair share i, so this exit is pair-uniform
  if (i >= n) return;
  typedef Fp2L28<C> E2;
  const MillerGroupAt at(mg, i);
  const int ppp = at.count;
  Fp28<C> px[MAXP], py[MAXP];
  bool live[MAXP];
  PreparedLines28<C> ls;
  ls.tab = pv.t28;
  for (int k = 0; k < 4; k++) ls.q[k] = k < ppp ? pv.q_of(at.slot, k) : 0u;
  ls.hi = lane_is_hi() ? 1 : 0;
  prepared_load_g1<C, MAXP>(px, py, live, pv, g1, at.first, ppp, ls.q);
  Fp12<C, E2> f, r;
  miller_loop_prepared_core<C, MAXP, E2, Fp28<C>>(f, px, py, live, ppp, ls);
  if (WHAT == 0) {
    lp28_store_gt<C>(out, i, f);
  } else {
    final_exp<C>(r, f);
    lp28_store_gt<C>(out, i, r);
  }
}

// four lanes per product (pairing_quad.h): the shorter dependent chain for batches that leave the chip under-filled
template <class C, int WHAT, int MAXP>
__global__ void __launch_bounds__(64) MLHIP_LP_OCC k_pairing_prep_q28(PreparedView<C> pv,
                                                                      const Affine<FpField<C>>* __restrict__ g1,
                                                                      MillerGroups mg, size_t n, Fp12<C>* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 2;  // the four lanes of a quad share i: quad-uniform exit
  if (i >= n) return;
  typedef Fp2L28<C> E2;
  const MillerGroupAt at(mg, i);
  const int ppp = at.count;
  Fp28<C> px[MAXP], py[MAXP];
  bool live[MAXP];
  PreparedLines28<C> ls;
  ls.tab = pv.t28;
  for (int k = 0; k < 4; k++) ls.q[k] = k < ppp ? pv.q_of(at.slot, k) : 0u;
  ls.hi = lane_is_hi() ? 1 : 0;
  prepared_load_g1<C, MAXP>(px, py, live, pv, g1, at.first, ppp, ls.q);
  Fp12Q<C, E2> f, r;
  miller_loop_prepared_q<C, MAXP, E2, Fp28<C>>(f, px, py, live, ppp, ls);
  if (WHAT != 0) {
    final_exp_q<C>(r, f);
    f = r;
  }
  q28_store_gt<C>(out, i, f);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
template <class C>
int g2_prepared_build(mlhip_g2_prepared_tables* t, hipStream_t st) {
  const size_t m = t->m;
  HIPCHK(hipMalloc((void**)&t->d_t28, m * prepared_words28<C>() * sizeof(int32_t)));
  HIPCHK(hipMalloc((void**)&t->d_inf, m * sizeof(uint32_t)));
  if constexpr (kBuildAlt) HIPCHK(hipMalloc(&t->d_t32, m * prepared_num_lines<C>() * sizeof(Line<C, Fp2<C>>)));
  k_g2_prepare<C><<<dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st>>>((const Affine<Fp2Field<C>>*)t->d_q, m, t->d_t28,
                                                                       (Line<C, Fp2<C>>*)t->d_t32, t->d_inf);
  HIPCHK(hipGetLastError());
  return 0;
}

// Which kernels run a batch (what: 0 = Miller loop, 2 = Miller loop + final exponentiation):
//   * MLHIP_PAIRING_ONE_LANE=1 (test build): one lane per product over the boundary-form table;
//   * quads while the batch leaves the chip under-filled, lane pairs above: pairing_wants_quads (pairing_kernels.h), the
//     switch of the general kernels (MLHIP_PAIRING_QUAD=1 / 0 forces / forbids the quads);
//   * MLHIP_G2_PREPARED_GENERAL=1, or a size inside prepared_general_range(): the GENERAL kernels on the Qs expanded from
//     the handle's affine copy -- where the measured A/B (tools/perf_g2_prepared.py) says they win
//     (MLHIP_G2_PREPARED_GENERAL=0 keeps the prepared kernels at every size).
// [lo, hi): the batch sizes at which the general kernels run, per curve, what and ppp.  EMPTY on every curve: in
// profiles/g2_prepared_ab.txt (DESIGN.md section 10 has the table) the prepared kernels are ahead of the general entry points
// at every grid point, and the fallback itself (expanding the Qs, then the general kernels) is nowhere ahead of them beyond
// the spread.
struct PreparedGeneralRange {
  size_t lo, hi;
};
template <class C>
PreparedGeneralRange prepared_general_range(int what, size_t ppp) {
  (void)what;
  (void)ppp;
  return {0, 0};
}

template <class C, class General>
int g2_prepared_run(const mlhip_g2_prepared_tables* t, int what, const void* d_g1, const uint32_t* q_index, size_t ppp,
                    size_t n, void* d_out, hipStream_t st, General general, const MillerGroups* groups = nullptr,
                    const uint32_t* d_index = nullptr) {
  if (n == 0) return 0;
  // groups: the n Miller loops are the groups of longer products (pairing_products.h; what = 0, ppp = the pairs of a full
  // group, q_index unused: slot s of every product pairs with Q[d_index[s]], a device array); without it, loop i takes
  // the ppp pairs from i ppp against Q[q_index[0 .. ppp)]
  const MillerGroups mg = groups ? *groups : miller_groups_plain(ppp);
  typedef Affine<FpField<C>> A1;
  typedef Affine<Fp2Field<C>> A2;
  PreparedView<C> pv;
  pv.t28 = t->d_t28;
  pv.t32 = (const Line<C, Fp2<C>>*)t->d_t32;
  pv.q_inf = t->d_inf;
  for (size_t j = 0; j < 4; j++) pv.q[j] = j < ppp && !groups ? (q_index ? q_index[j] : (uint32_t)j) : 0u;
  pv.d_index = groups ? d_index : nullptr;
  Fp12<C>* out = (Fp12<C>*)d_out;
  const A1* g1 = (const A1*)d_g1;
  const char* ge = getenv("MLHIP_G2_PREPARED_GENERAL");
  const PreparedGeneralRange gr = prepared_general_range<C>(what, ppp);
  if (!groups && (ge ? ge[0] == '1' : (n >= gr.lo && n < gr.hi))) {
    // scratch of this call alone: the handle stays read-only, so concurrent callers need no lock.  hipMalloc / hipFree make
    // this path synchronous: the call returns when its work is done (include/mlhip.h says so)
    A2* d_q = nullptr;
    Fp12<C>* d_f = nullptr;
    HIPCHK(hipMalloc((void**)&d_q, n * ppp * sizeof(A2)));
    int rc = 0;
    k_g2_prepared_expand<C><<<dim3((unsigned)((n * ppp + 255) / 256)), dim3(256), 0, st>>>((const A2*)t->d_q, pv, (int)ppp, n, d_q);
    if (hipGetLastError() != hipSuccess) rc = mlhip_rt::fail(MLHIP_EHIP, "k_g2_prepared_expand: launch failed");
    if (!rc) {
      if (what == 0 || ppp == 1) {
        rc = general(what, g1, d_q, ppp, n, nullptr, d_out, st);
      } else if (hipMalloc((void**)&d_f, n * sizeof(Fp12<C>)) != hipSuccess) {
        rc = mlhip_rt::fail(MLHIP_ENOMEM, "hipMalloc of the Miller values failed");
      } else {
        rc = general(0, g1, d_q, ppp, n, nullptr, d_f, st);
        if (!rc) rc = general(1, nullptr, nullptr, 1, n, d_f, d_out, st);
      }
    }
    // hipFree waits for the work that uses the buffers
    (void)hipFree(d_q);
    if (d_f) (void)hipFree(d_f);
    return rc;
  }
  if (mlhip_alt_switch("MLHIP_PAIRING_ONE_LANE")) {
    if constexpr (kBuildAlt) {
      const unsigned blocks = (unsigned)((n + 63) / 64);
      if (what == 0)
        k_miller_prepared<C, 0><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
      else
        k_miller_prepared<C, 2><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (pairing_wants_quads<C>(what, n)) {
    const unsigned blocks = (unsigned)((4 * n + 63) / 64);
    if (what == 0 && ppp == 1)
      k_pairing_prep_q28<C, 0, 1><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    else if (what == 0)
      k_pairing_prep_q28<C, 0, 4><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    else if (ppp == 1)
      k_pairing_prep_q28<C, 2, 1><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    else
      k_pairing_prep_q28<C, 2, 4><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
  } else {
    const unsigned blocks = (unsigned)((2 * n + 63) / 64);
    if (what == 0 && ppp == 1)
      k_pairing_prep_lp28<C, 0, 1><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    else if (what == 0)
      k_pairing_prep_lp28<C, 0, 4><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    else if (ppp == 1)
      k_pairing_prep_lp28<C, 2, 1><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
    else
      k_pairing_prep_lp28<C, 2, 4><<<dim3(blocks), dim3(64), 0, st>>>(pv, g1, mg, n, out);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace mlhip
