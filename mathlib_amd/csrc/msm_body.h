// msm_body.h -- per-thread bodies of the Pippenger MSM kernels (gfx950), shared with the host-side
// emulation used by tests/test_host_math.py (each body is __host__ __device__ and takes the global
// thread index explicitly, so the CPU test can replay a launch thread by thread).
//
// Replaces gnark-crypto's MultiExp behind the reference's MultiScalarMul
// (driver/gurvy/bls12381/bls12-381.go:766-783, driver/gurvy/bn254.go:232-245,
// driver/gurvy/bls12-377.go:229-242): signed-digit windows, bucket accumulation in XYZZ
// coordinates, bucket reduction, window combination.  Data layout and pipeline: DESIGN.md section 3.
#pragma once
#include <cstring>

#include "ec.h"

namespace mlhip {

// Signed 4-bit windows of a 256-bit integer: s + 0x88..8 has the nibbles d_w + 8 with d_w in [-8, 7] and
// s = sum_w d_w 16^w + t[8] 16^64 (t[8] = the carry out of the addition: 0 for a scalar below 2^255).  The carries of the
// recoding are the carries of one 256-bit addition -- no per-window branch; the table holds {1..8}P, half of the
// unsigned form's, and every lane of a wave adds at the same loop positions (a windowed NAF would not: its non-zero
// digits sit at data-dependent positions, which serialises the lanes).
MLHIP_HD void signed_windows4(uint32_t t[9], const uint32_t s[8]) {
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    c += (uint64_t)s[k] + 0x88888888u;
    t[k] = (uint32_t)c;
    c >>= 32;
  }
  t[8] = (uint32_t)c;
}
MLHIP_HD int signed_window4_digit(const uint32_t t[9], int w) {
  return w == 64 ? (int)t[8] : (int)((t[w >> 3] >> ((w & 7) * 4)) & 15u) - 8;
}

// ---- scalar handling -------------------------------------------------------------------------
// Scalars arrive as 8 little-endian 32-bit words: either gnark's fr.Element (Montgomery, R = 2^256;
// what driver/gurvy/bls12381 passes, bls12-381.go:772) or a plain integer (any 256-bit value; it is
// reduced mod r here, as fr.Element.SetBigInt does for the BaseZr curves, bn254.go:239).
template <class C>
MLHIP_HD void fr_canonical(uint32_t (&s)[8], const uint32_t* in, bool mont) {
  uint32_t t[9];
#pragma unroll
  for (int i = 0; i < 8; i++) t[i] = in[i];
  t[8] = 0;
  if (mont) {
    // Montgomery reduction: t <- t * 2^-256 mod r
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint32_t m = t[0] * C::FR_INV;
      uint64_t acc = (uint64_t)m * C::FR[0] + t[0];
      uint64_t c = acc >> 32;
#pragma unroll
      for (int j = 1; j < 8; j++) {
        acc = (uint64_t)m * C::FR[j] + t[j] + c;
        t[j - 1] = (uint32_t)acc;
        c = acc >> 32;
      }
      acc = (uint64_t)t[8] + c;
      t[7] = (uint32_t)acc;
      t[8] = (uint32_t)(acc >> 32);
    }
  }
  // reduce below r (a 256-bit input is < 16 r for every supported curve)
  for (int it = 0; it < 16; it++) {
    uint32_t d[8];
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint64_t x = (uint64_t)t[i] - C::FR[i] - br;
      d[i] = (uint32_t)x;
      br = (x >> 32) & 1;
    }
    bool ge = (t[8] != 0) | (br == 0);
    if (!ge) break;
    t[8] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = d[i];
  }
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = t[i];
}

// Short-scalar plans (mlhip_msm_plan_create_bits): the canonical value masked to its low `bits` bits -- the one place that
// does it, for the device kernels, the host build and the tests alike.  bits >= FR_BITS leaves the value as it is (a
// canonical scalar is below r < 2^FR_BITS), so full-width plans pass C::FR_BITS and pay one compare.
MLHIP_HD void fr_mask_bits(uint32_t (&s)[8], int bits) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int lo = 32 * i;
    if (bits <= lo)
      s[i] = 0;
    else if (bits < lo + 32)
      s[i] &= (1u << (bits - lo)) - 1u;
  }
}
template <class C>
MLHIP_HD void fr_canonical_bits(uint32_t (&s)[8], const uint32_t* in, bool mont, int bits) {
  fr_canonical<C>(s, in, mont);
  if (bits < C::FR_BITS) fr_mask_bits(s, bits);
}

// Effective window width of a plan over `bits`-bit scalars asked for width c: W = ceil((bits + 1) / c) windows need only
// c' = ceil((bits + 1) / W) <= c bits each, and ceil((bits + 1) / c') = W again, so the balanced layout under c' is the
// same W windows with 2^(c'-1) buckets instead of 2^(c-1).  Only short-scalar plans are normalised this way: a full-width
// plan keeps the c it was asked for (its geometry is what it always was).
MLHIP_HD int msm_effective_c(int bits, int c) {
  const int W = (bits + c) / c;
  return (bits + W) / W;
}

MLHIP_HD int msm_num_windows(int fr_bits, int c) { return (fr_bits + 1 + c - 1) / c; }

// Window layout.  The FR_BITS + 1 bits of a scalar (the extra bit absorbs the last carry) are spread over
// W = ceil((FR_BITS + 1) / c) windows as evenly as possible: the first `rem` windows are base + 1 bits wide, the others
// base bits, base = (FR_BITS + 1) / W.  For 256 = 16 x 16 bits (BLS12-381 at c = 16) every window is c bits; where c
// does not divide -- BLS12-377 and BN254 at c = 16 (254 / 255 bits), every curve at other widths -- this replaces a full
// set of c-bit windows plus a sparse top window, whose few buckets were several times longer than all the others (one
// thread per bucket: the accumulation waited for them), by windows that differ by one bit.
struct WinLayout {
  int W, base, rem;
};
MLHIP_HD WinLayout msm_win_layout(int fr_bits, int c) {
  WinLayout l;
  l.W = msm_num_windows(fr_bits, c);
  l.base = (fr_bits + 1) / l.W;
  l.rem = (fr_bits + 1) % l.W;
  return l;
}
MLHIP_HD int msm_win_off(int wbase, int wrem, int w) { return w * wbase + (w < wrem ? w : wrem); }
MLHIP_HD int msm_win_bits(int wbase, int wrem, int w) { return wbase + (w < wrem ? 1 : 0); }

// The Horner pass of the host tail (msm_plan.h: host_tail): down[w] = doublings between window w and window w - 1 of the
// layout over `bits` + 1 bits (down[0] = 0); their sum is off(W - 1), below the plan's scalar width.
inline void msm_window_shifts(int bits, int c, int* down /* [W] */) {
  const WinLayout wl = msm_win_layout(bits, c);
  down[0] = 0;
  for (int w = 1; w < wl.W; w++) down[w] = msm_win_off(wl.base, wl.rem, w) - msm_win_off(wl.base, wl.rem, w - 1);
}

// Signed digit of window w: v = bits [off, off + width) + carry; v > 2^(width-1) => v -= 2^width, carry 1.
// Returns the magnitude (0 = skip; bucket = magnitude - 1), sets neg and the carry into the next window.
MLHIP_HD uint32_t msm_window_digit(const uint32_t (&s)[8], int off, int width, uint32_t& carry, uint32_t& neg) {
  uint32_t v = 0;
  if (off < 256) {
    const int word = off >> 5, sh = off & 31;
    uint64_t two = s[word];
    if (word + 1 < 8) two |= (uint64_t)s[word + 1] << 32;
    v = (uint32_t)((two >> sh) & ((1u << width) - 1));
  }
  v += carry;
  const uint32_t half = 1u << (width - 1);
  if (v > half) {
    // v == 2^width (all-ones window plus carry) is digit 0 with a carry, not "minus zero"
    carry = 1;
    neg = 1;
    return (1u << width) - v;
  }
  carry = 0;
  neg = 0;
  return v;
}

// windows of a signed w-bit fixed-base table (msm_scalar_mul.h, msm_bases_batch.h): ceil(256 / w)
MLHIP_HD int fb_windows(int w) { return (256 + w - 1) / w; }

// Encoded as 0 (skip) or (magnitude << 1) | sign with magnitude in [1, 2^(width-1)] -> bucket magnitude-1.
template <class C>
// (`bits`: the plan's scalar width -- the layout covers bits + 1 bits and the value is masked to `bits`)
MLHIP_HD void msm_digits_body(size_t i, size_t n, const uint32_t* scalars, bool mont, int c, int W,
                              uint32_t* digits /* [W][n] */, int bits = C::FR_BITS) {
  uint32_t s[8];
  fr_canonical_bits<C>(s, scalars + 8 * i, mont, bits);
  const WinLayout l = msm_win_layout(bits, c);
  uint32_t carry = 0, neg = 0;
  for (int w = 0; w < W; w++) {
    const uint32_t mag = msm_window_digit(s, msm_win_off(l.base, l.rem, w), msm_win_bits(l.base, l.rem, w), carry, neg);
    digits[(size_t)w * n + i] = mag ? ((mag << 1) | neg) : 0u;
  }
}

// ---- bucket accumulation ---------------------------------------------------------------------
// One thread owns bucket g = w*M + b: adds the points listed in sorted[offset .. offset+count).
template <class F>
MLHIP_HD void msm_accumulate_range(XYZZ<F>& acc, const Affine<F>* points, const uint32_t* sorted, size_t begin,
                                   size_t end, size_t stride) {
  if (begin >= end) return;
  // software prefetch: the next entry's index and point are loaded before the current mixed addition,
  // so the two dependent gathers (index, then a random 96/192-byte row) overlap ~30k cycles of arithmetic
  uint32_t e = sorted[begin];
  Affine<F> p = points[e & 0x7fffffffu];
  for (size_t k = begin; k < end; k += stride) {
    const size_t kn = k + stride;
    uint32_t en = e;
    Affine<F> pn = p;
    if (kn < end) {
      en = sorted[kn];
      pn = points[en & 0x7fffffffu];
    }
    xyzz_madd<F>(acc, p, (e >> 31) != 0);
    e = en;
    p = pn;
  }
}

// ---- bucket reduction, level 1 ---------------------------------------------------------------
// Chunk g of window w owns buckets [g L, (g + 1) L): A = sum_i b[i], W0 = sum_i i b[i], as a running sum from the top
// bucket down (acc += b[i]; w0 += acc; the last acc += b[0] adds nothing to w0).  Written once, over a reduction form R
// (msm_reduce.h: "reduction forms"), which is the only place that knows how a point is kept, and the group addition
// `add(acc, q)`: the kernels pass their form's (FormAdd), the host test the host backends of the quad and lane-pair
// additions.  R::CHUNK_PREFETCH: the next bucket is loaded under the additions of this one (a second value stays live).
template <class R, class AddFn>
MLHIP_HD void reduce_chunk_body(size_t g, const typename R::Mem* buckets, typename R::Mem* A, typename R::Mem* W0, int l_eff,
                                AddFn add) {
  const typename R::Mem* b = buckets + R::MEMS * g * (size_t)l_eff;
  typename R::V acc, w0, cur;
  R::set_empty(acc);
  R::set_empty(w0);
  if constexpr (R::CHUNK_PREFETCH) R::load(cur, b, l_eff - 1);
#pragma unroll 1
  for (int i = l_eff - 1; i >= 0; i--) {
    [[maybe_unused]] typename R::V nxt;  // (the prefetched bucket: not used without CHUNK_PREFETCH)
    if constexpr (R::CHUNK_PREFETCH) {
      nxt = cur;
      if (i > 0) R::load(nxt, b, i - 1);
    } else {
      R::load(cur, b, i);
    }
    add(acc, cur);
    if (i > 0) add(w0, acc);
    if constexpr (R::CHUNK_PREFETCH) cur = nxt;
  }
  R::store(A, g, acc);
  R::store(W0, g, w0);
}

// The same with one point per lane in the boundary form and the addition passed in: the ordering every form's chunk sums
// reproduce, which the host test drives with xyzz_add itself.
template <class F>
struct ChunkLaneForm {
  static constexpr bool CHUNK_PREFETCH = false;
  static constexpr int MEMS = 1;
  typedef XYZZ<F> Mem, V;
  MLHIP_HD static void set_empty(V& v) { xyzz_set_inf<F>(v); }
  MLHIP_HD static void load(V& v, const Mem* arr, size_t i) { v = arr[i]; }
  MLHIP_HD static void store(Mem* arr, size_t i, const V& v) { arr[i] = v; }
};
template <class F, class AddFn>
MLHIP_HD void msm_chunk_body(size_t g, const XYZZ<F>* buckets, XYZZ<F>* A, XYZZ<F>* W0, int l_eff, AddFn add) {
  reduce_chunk_body<ChunkLaneForm<F>>(g, buckets, A, W0, l_eff, add);
}

// ---- bucket reduction, level 2: which chunk sums make up the nsel = 4 + log2 T sums of a window ------------------------
// List sel of a window with T chunks (T a power of two): sel 0, 1 -> the two halves of sum_t W0[t]; sel 2, 3 -> the two
// halves of sum_t A[t] (split at (T + 1) / 2); sel 4 + k -> the A[t] with bit k of t set.  Every list of T >= 2 has T / 2
// elements (equal depth); at T = 1 the second halves are empty.  reduce_sel_index: element j of list sel -> t.
MLHIP_HD uint32_t reduce_sel_count(int sel, uint32_t T) {
  const uint32_t half = (T + 1) / 2;
  return sel >= 4 ? T / 2 : (sel & 1) ? T - half : half;
}
MLHIP_HD uint32_t reduce_sel_index(int sel, uint32_t j, uint32_t T) {
  const int k = sel < 4 ? 0 : sel - 4;
  const uint32_t lo = (sel & 1) ? (T + 1) / 2 : 0u;
  return sel < 4 ? lo + j : (((j >> k) << (k + 1)) | (1u << k) | (j & ((1u << k) - 1u)));
}

// ---- host tail of one window (msm_plan.h: host_tail; here so that the host-math test library can run it) ------------
// V = out[0..3] summed + 2^lgL sum_k 2^k out[4 + k]: nb + lgL doublings and nb + 4 additions
struct HostTailHeader {
  int nb, lgL, nsel, pad;
};
template <class F>
void host_tail_window(const void* in, int w, void* out) {
  const HostTailHeader& h = *static_cast<const HostTailHeader*>(in);
  const XYZZ<F>* o = reinterpret_cast<const XYZZ<F>*>(static_cast<const unsigned char*>(in) + sizeof(HostTailHeader)) + (size_t)w * h.nsel;
  XYZZ<F> acc, d;
  xyzz_set_inf<F>(acc);
  for (int k = h.nb - 1; k >= 0; k--) {
    xyzz_dbl<F>(d, acc);
    acc = d;
    xyzz_add<F>(acc, o[4 + k]);
  }
  for (int k = 0; k < h.lgL; k++) {
    xyzz_dbl<F>(d, acc);
    acc = d;
  }
  for (int q = 0; q < 4; q++) xyzz_add<F>(acc, o[q]);
  memcpy(out, &acc, sizeof(acc));
}

}  // namespace mlhip
