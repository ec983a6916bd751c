// gt_codec.h -- what a Gt value needs besides Mul and Exp: the membership test behind mlhip_gt_is_member and the checking
// decoder, Gt.Inverse, and the kernels of gnark's GT.Bytes() wire format.  Included at the end of
// pairing_kernels.h; the chains above the kernels are host-testable (tests/hostmath_gtcodec).
//
// Membership.  f lies in Gt (f^r = 1) if and only if
//     (0)  f != 0
//     (i)  frob^2(frob^2(f)) f == frob^2(f)            f^(p^4 - p^2 + 1) = 1: f is in the cyclotomic subgroup
//     (ii) frob(f) == f^lambda                         lambda = x (BLS12; the conjugate of f^|x| for x < 0), 6 x^2 (BN254)
// because gcd(Phi_12(p), p - lambda) = r: on BLS12, Phi_12(p) mod (p - x) = Phi_12(x) = r and r | p - x; on BN254
// p - 6 x^2 = r itself.  f^lambda is computed with Granger-Scott squarings, which are only squarings on values that passed
// (i): all three verdicts are computed on every input and ANDed -- no branch depends on the data, and an arbitrary Fp12
// value (0 included) is straight-line field arithmetic, as in gt_exp_cyclo.h.
// Comparisons are made on CANONICAL values: both sides go through fp28_to_fp, the conversion the kernels store their results
// with (one product and the representative in [0, p)), and the 32-bit limbs are compared.
#pragma once
#include <type_traits>

#include "gt_exp_cyclo.h"

namespace mlhip {

// AND of a per-lane verdict over the LANES (2: a pair, 4: a quad) that hold one value; the host models hold every lane
template <int LANES>
MLHIP_HD bool gt_all_lanes(bool ok) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t z = ok ? 1u : 0u;
  z &= pair_xchg_u32(z);
  if (LANES == 4) z &= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)z, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
  return z != 0;
#else
  return ok;
#endif
}

// the canonical boundary form of this lane's component i of coefficient e
template <class C, class E>
MLHIP_HD void gt_canon(Fp<C>& r, const E& e, int i) {
  E::require(e.w() <= LP28_MAXW && e.vb() <= LP28_MAXU, "gt_canon (weight, value bound)", e.w(), e.vb());
  fp28_to_fp<C>(r, e.at(i));
}
template <class C, class G>
MLHIP_HD bool gt_eq(const typename G::T& a, const typename G::T& b) {
  const auto* x = G::coeffs(a);
  const auto* y = G::coeffs(b);
  typedef typename std::remove_cv<typename std::remove_pointer<decltype(x)>::type>::type E;
  bool ok = true;
#pragma unroll 1
  for (int k = 0; k < G::COEFFS; k++)
    for (int i = 0; i < E::LANES; i++) {
      Fp<C> u, v;
      gt_canon<C>(u, x[k], i);
      gt_canon<C>(v, y[k], i);
      ok &= fp_eq<C>(u, v);
    }
  return gt_all_lanes<G::DEVICE_LANES>(ok);
}
template <class C, class G>
MLHIP_HD bool gt_is_zero(const typename G::T& a) {
  const auto* x = G::coeffs(a);
  typedef typename std::remove_cv<typename std::remove_pointer<decltype(x)>::type>::type E;
  bool ok = true;
#pragma unroll 1
  for (int k = 0; k < G::COEFFS; k++)
    for (int i = 0; i < E::LANES; i++) {
      Fp<C> u;
      gt_canon<C>(u, x[k], i);
      ok &= fp_is_zero<C>(u);
    }
  return gt_all_lanes<G::DEVICE_LANES>(ok);
}

// r = z^|x| by cyclotomic squarings: 62 / 63 squarings and popcount(|x|) - 1 products; the branch depends on the seed only
template <class C, class G>
MLHIP_HD void gt_pow_seed(typename G::T& r, const typename G::T& z) {
  int top = 63;
  while (!((C::X_ABS >> top) & 1)) top--;
  typename G::T acc = z;
#pragma unroll 1
  for (int i = top - 1; i >= 0; i--) {
    G::cyclo_sqr(acc, acc);
    if ((C::X_ABS >> i) & 1) G::mul(acc, acc, z);
  }
  r = acc;
}

// f in Gt?  (the same verdict on every lane that holds f)
template <class C, class G>
MLHIP_HD bool gt_is_member_chain(const typename G::T& f) {
  typename G::T a, b, c;
  G::template frob<2>(a, f);
  G::template frob<2>(b, a);
  G::mul(c, b, f);
  const bool cyclotomic = gt_eq<C, G>(c, a);
  const bool nonzero = !gt_is_zero<C, G>(f);
  gt_pow_seed<C, G>(c, f);
  if constexpr (C::IS_BN) {
    gt_pow_seed<C, G>(b, c);  // f^(x^2)
    G::cyclo_sqr(c, b);
    G::cyclo_sqr(b, c);
    G::mul(c, c, b);  // ^2 ^4: f^(6 x^2)
  } else if (C::X_NEG) {
    G::conj(c, c);
  }
  G::template frob<1>(a, f);
  const bool eigen = gt_eq<C, G>(c, a);
  return nonzero & cyclotomic & eigen;
}

#if defined(__HIPCC__)
}  // namespace mlhip
#include "codec.h"
namespace mlhip {

// ---- wire format: 12 big-endian Fp values, C1.B2.A1 first -- wire coordinate k is memory coordinate 11 - k ----------------
// One COORDINATE per lane, 12 lanes per value, 16 values per 192-lane block: a lane moves fp bytes, neighbouring lanes
// neighbouring coordinates, so a block reads and writes one contiguous stretch in both directions (with one value per lane,
// as the point codecs have it, neighbouring lanes would sit 576 bytes apart).  The verdict of a value is the OR over its 12
// lanes, which straddle waves: one LDS word per value.
constexpr int GT_CODEC_VALUES = 16, GT_CODEC_BLOCK = 12 * GT_CODEC_VALUES;

template <class C>
__global__ void __launch_bounds__(GT_CODEC_BLOCK) k_gt_decode(const uint8_t* __restrict__ wire, size_t n, Fp<C>* __restrict__ out,
                                                              uint8_t* __restrict__ status) {
  __shared__ uint32_t bad[GT_CODEC_VALUES];
  const unsigned e = threadIdx.x / 12u, k = threadIdx.x - 12u * e;
  if (threadIdx.x < GT_CODEC_VALUES) bad[threadIdx.x] = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * GT_CODEC_VALUES + e;
  const bool live = i < n;
  Fp<C> v, zero;
  fp_zero<C>(v);
  fp_zero<C>(zero);
  if (live) {
    if (!fp_from_be<C>(v, wire + (i * 12 + k) * (size_t)(4 * C::N), 0xFF)) bad[e] = 1;  // (every writer stores the same word)
    fp_to_mont<C>(v, v);
  }
  __syncthreads();
  if (live) {
    const bool good = bad[e] == 0;
    fp_select<C>(v, good, v, zero);
    out[i * 12 + (11 - k)] = v;
    if (k == 0) status[i] = good ? (uint8_t)CODEC_OK : (uint8_t)CODEC_MALFORMED;
  }
}

template <class C>
__global__ void __launch_bounds__(GT_CODEC_BLOCK) k_gt_encode(const Fp<C>* __restrict__ in, size_t n, uint8_t* __restrict__ wire) {
  const size_t t = (size_t)blockIdx.x * GT_CODEC_BLOCK + threadIdx.x;
  const size_t i = t / 12;
  if (i >= n) return;
  const unsigned k = (unsigned)(t - 12 * i);
  Fp<C> v = in[i * 12 + (11 - k)];
  fp_from_mont<C>(v, v);
  fp_to_be<C>(wire + t * (size_t)(4 * C::N), v);
}

// ---- membership and inverse over GtShape (pairing_kernels.h), launched by gt_launch
// status[i] = in[i] in Gt ? 0 : 3.  With `decoded` (the second launch of a checking mlhip_gt_from_bytes: in == decoded) a
// status the decoder set stays, and a value that fails the test is overwritten with zeros.
template <class C, bool QUAD>
__global__ void __launch_bounds__(64) MLHIP_LP_OCC k_gt_member(const Fp12<C>* in, size_t n, uint8_t* status, Fp12<C>* decoded) {
  typedef GtShape<C, QUAD> S;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t / S::LANES;  // uniform over the lanes of one value
  if (i >= n) return;
  typename S::T f;
  S::load(f, in, i);
  uint8_t s = gt_is_member_chain<C, typename S::G>(f) ? (uint8_t)CODEC_OK : (uint8_t)CODEC_NOT_IN_SUBGROUP;
  if (decoded) {
    const uint8_t prev = status[i];
    s = prev ? prev : s;
    if (s) {
      S::zero(f);
      S::store(decoded, i, f);
    }
  }
  if ((threadIdx.x & (S::LANES - 1)) == 0) status[i] = s;
}

// out[i] = 1 / in[i] for any Fp12 value; 1 / 0 = 0 (the divsteps inversion maps 0 to 0 in a fixed number of steps)
template <class C, bool QUAD>
__global__ void __launch_bounds__(64) MLHIP_LP_OCC k_gt_inverse(const Fp12<C>* in, size_t n, Fp12<C>* out) {
  typedef GtShape<C, QUAD> S;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t / S::LANES;
  if (i >= n) return;
  typename S::T f, r;
  S::load(f, in, i);
  S::G::inv(r, f);
  S::store(out, i, r);
}

template <class C>
int gt_is_member_device(const void* d_in, size_t n, void* d_status, void* d_decoded, hipStream_t st) {
  return gt_launch<C>(k_gt_member<C, true>, k_gt_member<C, false>, n, st, (const Fp12<C>*)d_in, n, (uint8_t*)d_status,
                      (Fp12<C>*)d_decoded);
}

template <class C>
int gt_inverse_device(const void* d_in, size_t n, void* d_out, hipStream_t st) {
  return gt_launch<C>(k_gt_inverse<C, true>, k_gt_inverse<C, false>, n, st, (const Fp12<C>*)d_in, n, (Fp12<C>*)d_out);
}

// decode, then -- with the check -- the membership kernel over the decoded values on the same stream (two launches: the
// decoder wants a lane per coordinate, the test a quad per value)
template <class C>
int gt_decode_device(const void* d_wire, size_t n, int subgroup_check, void* d_out, void* d_status, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + GT_CODEC_VALUES - 1) / GT_CODEC_VALUES);
  k_gt_decode<C><<<dim3(blocks), dim3(GT_CODEC_BLOCK), 0, st>>>((const uint8_t*)d_wire, n, (Fp<C>*)d_out, (uint8_t*)d_status);
  HIPCHK(hipGetLastError());
  if (subgroup_check) return gt_is_member_device<C>(d_out, n, d_status, d_out, st);
  return 0;
}

template <class C>
int gt_encode_device(const void* d_in, size_t n, void* d_wire, hipStream_t st) {
  const unsigned blocks = (unsigned)((12 * n + GT_CODEC_BLOCK - 1) / GT_CODEC_BLOCK);
  k_gt_encode<C><<<dim3(blocks), dim3(GT_CODEC_BLOCK), 0, st>>>((const Fp<C>*)d_in, n, (uint8_t*)d_wire);
  HIPCHK(hipGetLastError());
  return 0;
}
#endif  // __HIPCC__

}  // namespace mlhip
