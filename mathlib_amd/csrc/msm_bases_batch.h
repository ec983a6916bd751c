// msm_bases_batch.h -- many independent small MSMs over the resident bases of a mlhip_bases handle
// (mlhip_bases_msm_batch*): out[k] = sum over segment k of [s_i] B[idx(i)].  Part of msm_kernels.h; the per-lane body above
// the kernels is plain C++ / __host__ __device__, so tests/hostmath_bases_batch replays it on the CPU.  Cost model and
// measurements: DESIGN.md section 9.
//
//   tables     per base b of the handle, T_b[j][m - 1] = [m 2^(wj)] B_b, m = 1 .. 2^(w-1), j < ceil(256 / w): the one-base
//              layout of msm_scalar_mul.h stacked base after base, in the carry-free form the product kernel reads (Affine28
//              rows for G1, AffineG2_28 for G2).  Built on the device by k_fb_scalars + k_scalar_mul(_lp) (entry t of a
//              build belongs to base t / entries) the first time a call needs them, extended when a later call needs more
//              bases, owned and freed by the handle.  At most MLHIP_BASES_BATCH_MAX_MB per handle: a call whose tables
//              would pass that takes the table-free path below (= 0: never any table).
//   chunks     the segments cut into chunks of at most P pairs (msm_batch_layout); one lane (G1) or lane pair (G2) per chunk
//              adds, for every pair, ceil(256 / w) entries +-T_idx[j][|d_j|] (signed w-bit digits of the reduced scalar,
//              msm_window_digit) into one XYZZ28 accumulator -- no doubling, no per-lane table -- and writes its partial
//              in XYZZ; the sum passes of msm_batch.h (k_msm_batch_sum / _lp) add the partials of each segment.
//   table-free the variable-base body of mlhip_msm_batch (msm_batch_chunk, its P) reading the handle's points by index; its long
//              segments take the bucket route of msm_batch_bucket.h (the same switches and per-group defaults), the point
//              of a pair read through the index list (MsmBucketIndexed).
#pragma once
#include <cstdint>
#include <cstdlib>

#include "ec28.h"
#include "ec28_lp.h"
#include "msm_batch.h"
#include "msm_batch_bucket.h"

namespace mlhip {

// defaults measured on an MI355X (profiles/bases_batch_grid.jsonl): the widest table wins every
// verifier-sized cell for 64 bases (fewer additions beat the extra cache misses), and the chunk length is the largest that
// still leaves BASES_BATCH_FILL_LANES lanes -- below that the device is not filled and shorter chains win
constexpr int BASES_BATCH_W_DEFAULT_G1 = 12, BASES_BATCH_W_DEFAULT_G2 = 12, BASES_BATCH_W_MIN = 4, BASES_BATCH_W_MAX = 12;
constexpr size_t BASES_BATCH_FILL_LANES = (size_t)1 << 16;
constexpr size_t BASES_BATCH_MAX_MB_DEFAULT = 1024;
inline bool bases_batch_p_valid(int p) { return p == 1 || p == 2 || p == 4 || p == 8 || p == 16; }
// table rows per base at width w
MLHIP_HD size_t bases_batch_entries(int w) { return (size_t)fb_windows(w) << (w - 1); }

// the accumulator and the mixed addition of the product body: G1 one lane (ec28.h), G2 one Fp2 component per lane (ec28_lp.h)
template <class Curve>
struct BasesBatchOpsG1 {
  typedef Curve C;
  typedef XYZZ28<C> Acc;
  typedef Affine28<C> Row;
  MLHIP_HD static void madd(Acc& acc, bool& inf, const Row& q, bool neg) { xyzz28_madd<C>(acc, inf, q, neg); }
};
template <class Curve, class B>
struct BasesBatchOpsLp {
  typedef Curve C;
  typedef XYZZ28L<typename B::V> Acc;
  typedef Affine28L<typename B::V> Row;
  MLHIP_HD static void madd(Acc& acc, bool& inf, const Row& q, bool neg) { xyzz28_lp_madd<C, B>(acc, inf, q, neg); }
};

// (acc, inf) = sum_{j < count} [s_j] B_{b_j} for one chunk: scalars = 8 words per pair (fr_canonical: Montgomery or plain, not
// necessarily reduced), b_j = index[j] (index != nullptr) or base0 + j, row(q, b, t) reads entry t of base b's table.  Every
// branch depends on the scalars alone (pair-uniform for G2).  The accumulator may equal +-the entry it adds (the same base
// twice, (B, s) beside (B, r - s)): the mixed additions take their exact path there.
template <class Ops, class Row>
MLHIP_HD void bases_batch_chunk(typename Ops::Acc& acc, bool& inf, const uint32_t* scalars, const uint32_t* index, uint32_t base0,
                                uint32_t count, bool mont, int w, Row row) {
  typedef typename Ops::C C;
  inf = true;
  const int nw = fb_windows(w);
#pragma unroll 1
  for (uint32_t j = 0; j < count; j++) {
    uint32_t s[8];
    fr_canonical<C>(s, scalars + 8 * j, mont);
    const uint32_t b = index ? index[j] : base0 + j;
    uint32_t carry = 0, neg = 0;
#pragma unroll 1
    for (int win = 0; win < nw; win++) {
      const uint32_t m = msm_window_digit(s, win * w, w, carry, neg);
      if (m) {
        typename Ops::Row q;
        row(q, b, ((uint32_t)win << (w - 1)) + m - 1);
        Ops::madd(acc, inf, q, neg != 0);
      }
    }
  }
}

#if defined(__HIPCC__)
// ---- kernels ---------------------------------------------------------------------------------------------------------
// index: the call's base indices (one per pair, nullptr: base0 + position in the chunk); per_base = bases_batch_entries(w)
template <class C>
__global__ void __launch_bounds__(64) k_bases_batch_chunk(const Affine28<C>* __restrict__ tab, size_t per_base, int w,
                                                          const uint32_t* __restrict__ scalars, int mont,
                                                          const uint32_t* __restrict__ index,
                                                          const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                          XYZZ<FpField<C>>* __restrict__ partials) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const MsmBatchChunk ch = chunks[c];
  XYZZ28<C> acc;
  bool inf;
  bases_batch_chunk<BasesBatchOpsG1<C>>(acc, inf, scalars + 8 * ch.first, index ? index + ch.first : nullptr, ch.base0, ch.count,
                                        mont != 0, w,
                                        [&](Affine28<C>& q, uint32_t b, uint32_t t) { q = tab[(size_t)b * per_base + t]; });
  XYZZ<FpField<C>> r;
  xyzz28_to<C>(r, acc, inf);
  partials[c] = r;
}

template <class C>
__global__ void __launch_bounds__(64) k_bases_batch_chunk_lp(const AffineG2_28<C>* __restrict__ tab, size_t per_base, int w,
                                                             const uint32_t* __restrict__ scalars, int mont,
                                                             const uint32_t* __restrict__ index,
                                                             const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                             XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  typedef PairDevice<C> B;
  const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair share the chunk
  if (c >= n_chunks) return;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchChunk ch = chunks[c];
  XYZZ28L<Fp28<C>> acc;
  bool inf;
  bases_batch_chunk<BasesBatchOpsLp<C, B>>(acc, inf, scalars + 8 * ch.first, index ? index + ch.first : nullptr, ch.base0,
                                           ch.count, mont != 0, w, [&](Affine28L<Fp28<C>>& q, uint32_t b, uint32_t t) {
                                             const AffineG2_28<C>* e = tab + ((size_t)b * per_base + t);
                                             q.x = e->c[hi];
                                             q.y = e->c[2 + hi];
                                           });
  XYZZ<FL> r;
  if (inf) {
    xyzz_set_inf<FL>(r);
  } else {
    fp28_to_fp<C>(r.x.v, acc.x);
    fp28_to_fp<C>(r.y.v, acc.y);
    fp28_to_fp<C>(r.zz.v, acc.zz);
    fp28_to_fp<C>(r.zzz.v, acc.zzz);
  }
  lp_store_xyzz<C>(partials, c, r, hi);
}

// the table-free path: mlhip_msm_batch's per-lane body over the handle's points, read by index
template <class C, int P>
__global__ void __launch_bounds__(64) k_msm_batch_chunk_bases(const Affine<FpField<C>>* __restrict__ points,
                                                              const uint32_t* __restrict__ scalars, int mont,
                                                              const uint32_t* __restrict__ index,
                                                              const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                              XYZZ<FpField<C>>* __restrict__ partials) {
  typedef FpField<C> F;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const MsmBatchChunk ch = chunks[c];
  if (ch.count > (uint32_t)P) return;  // a slice of a long segment: the bucket kernels write this row (msm_batch_bucket.h)
  XYZZ<F> acc;
  msm_batch_chunk<F, P, MsmBatchOpsG1<F>>(acc, scalars + 8 * ch.first, ch.count, mont != 0, [&](Affine<F>& p, int j) {
    p = points[index ? index[ch.first + j] : ch.base0 + (uint32_t)j];
  });
  partials[c] = acc;
}

template <class C, int P>
__global__ void __launch_bounds__(64) k_msm_batch_chunk_bases_lp(const Affine<Fp2Field<C>>* __restrict__ points,
                                                                 const uint32_t* __restrict__ scalars, int mont,
                                                                 const uint32_t* __restrict__ index,
                                                                 const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                                 XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (c >= n_chunks) return;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchChunk ch = chunks[c];
  if (ch.count > (uint32_t)P) return;  // a slice of a long segment (both lanes of the pair leave)
  XYZZ<FL> acc;
  msm_batch_chunk<FL, P, MsmBatchOpsLp<C>>(acc, scalars + 8 * ch.first, ch.count, mont != 0, [&](Affine<FL>& p, int j) {
    lp_load_affine<C>(p, points, index ? index[ch.first + j] : ch.base0 + (uint32_t)j, hi);
  });
  lp_store_xyzz<C>(partials, c, acc, hi);
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline int bases_batch_env_int(const char* name, int lo, int hi, int dflt) {
  if (const char* e = getenv(name)) {
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end != e && v >= lo && v <= hi) return (int)v;
  }
  return dflt;
}
// the table width of this call: MLHIP_BASES_BATCH_WINDOW (4 .. 12), else the group's default
template <class C, class F>
int bases_batch_window() {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  return bases_batch_env_int("MLHIP_BASES_BATCH_WINDOW", BASES_BATCH_W_MIN, BASES_BATCH_W_MAX,
                             kG1 ? BASES_BATCH_W_DEFAULT_G1 : BASES_BATCH_W_DEFAULT_G2);
}
// the chunk length of the table path: MLHIP_BASES_BATCH_CHUNK if it names an allowed one, else the largest allowed length
// whose chunks still occupy BASES_BATCH_FILL_LANES lanes (one per G1 chunk, two per G2 chunk), else 1
template <class C, class F>
int bases_batch_chunk_len(const uint64_t* offsets, size_t k) {
  constexpr size_t kLanes = std::is_same<F, FpField<C>>::value ? 1 : 2;
  const int v = bases_batch_env_int("MLHIP_BASES_BATCH_CHUNK", 1, 16, 0);
  if (bases_batch_p_valid(v)) return v;
  for (int P = 16; P > 1; P /= 2) {
    size_t chunks = 0;
    for (size_t s = 0; s < k; s++) chunks += (size_t)((offsets[s + 1] - offsets[s] + (uint64_t)P - 1) / (uint64_t)P);
    if (chunks * kLanes >= BASES_BATCH_FILL_LANES) return P;
  }
  return 1;
}
// the per-handle cap in bytes: MLHIP_BASES_BATCH_MAX_MB (0 = no tables), else BASES_BATCH_MAX_MB_DEFAULT
static inline size_t bases_batch_cap_bytes() {
  return (size_t)bases_batch_env_int("MLHIP_BASES_BATCH_MAX_MB", 0, 1 << 20, (int)BASES_BATCH_MAX_MB_DEFAULT) << 20;
}

// Tables of bases [0, n_new) at width w in t (which holds [0, t->n_tabled) at width t->w): a new buffer, the rows already
// built copied over (same width), the others built in tiles of bases on the device.  Synchronous: when it returns, any
// stream may read the tables.
template <class C, class F>
int bases_batch_grow(mlhip_bases_batch_tables* t, const void* d_pts, size_t n_new, int w, hipStream_t st) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  const size_t per = bases_batch_entries(w);
  const size_t row = kG1 ? sizeof(Affine28<C>) : sizeof(AffineG2_28<C>);
  const size_t keep = t->buf && t->w == w ? std::min(t->n_tabled, n_new) : 0;
  const size_t tile = std::max<size_t>(1, ((size_t)1 << 19) / per);  // bases per build step: <= 2^19 entries of scratch
  const size_t tile_entries = std::min(tile, n_new - keep) * per;
  char* nb = nullptr;
  char* tmp = nullptr;
  int rc = 0;
  auto fail = [&](int code, const char* what) {
    (void)hipGetLastError();
    rc = mlhip_rt::fail(code, what);
  };
  if (hipMalloc((void**)&nb, n_new * per * row) != hipSuccess) fail(MLHIP_ENOMEM, "bases batch: hipMalloc of the tables failed");
  // scratch: [a zero header (k_fb_scalars / k_scalar_mul's skip flag) | the per-base scalars | boundary-form rows of a tile]
  const size_t sc_off = FB_HEADER, pts_off = sc_off + ((per * 32 + 255) & ~(size_t)255);
  if (!rc && hipMalloc((void**)&tmp, pts_off + tile_entries * sizeof(Affine<F>)) != hipSuccess)
    fail(MLHIP_ENOMEM, "bases batch: hipMalloc of the table build's scratch failed");
  if (!rc && keep && hipMemcpyAsync(nb, t->buf, keep * per * row, hipMemcpyDeviceToDevice, st) != hipSuccess)
    fail(MLHIP_EHIP, "bases batch: copy of the tables failed");
  if (!rc && hipMemsetAsync(tmp, 0, FB_HEADER, st) != hipSuccess) fail(MLHIP_EHIP, "bases batch: hipMemsetAsync failed");
  if (!rc) {
    const uint32_t* zero = (const uint32_t*)tmp;
    uint32_t* tsc = (uint32_t*)(tmp + sc_off);
    Affine<F>* rows = (Affine<F>*)(tmp + pts_off);
    FbOrder order;
    for (int k = 0; k < 8; k++) order.w[k] = C::FR[k];
    k_fb_scalars<<<dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st>>>(tsc, w, (uint32_t)per, zero, order, 0);
    for (size_t b0 = keep; b0 < n_new; b0 += tile) {
      const size_t cnt = std::min(tile, n_new - b0), entries = cnt * per;
      const Affine<F>* src = (const Affine<F>*)d_pts + b0;
      if constexpr (kG1) {
        k_scalar_mul<C, F><<<dim3((unsigned)((entries + 63) / 64)), dim3(64), 0, st>>>(src, 0, tsc, -1, entries, rows, zero,
                                                                                       (uint32_t)per);
        k_fb_table_to28<C><<<dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st>>>(
            rows, entries, (Affine28<C>*)nb + b0 * per, zero, 0);
      } else {
        k_scalar_mul_lp<C><<<dim3((unsigned)((2 * entries + 63) / 64)), dim3(64), 0, st>>>(src, 0, tsc, -1, entries, rows, zero,
                                                                                        (uint32_t)per);
        k_points_to28_g2<C><<<dim3((unsigned)((4 * entries + 255) / 256)), dim3(256), 0, st>>>(rows, entries,
                                                                                             (AffineG2_28<C>*)nb + b0 * per);
      }
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) fail(MLHIP_EHIP, "bases batch: table build failed");
  }
  if (tmp) (void)hipFree(tmp);
  if (rc) {
    if (nb) (void)hipFree(nb);
    return rc;
  }
  if (t->buf) (void)hipFree(t->buf);  // waits for the device: no earlier call is still reading it
  t->buf = nb;
  t->n_tabled = n_new;
  t->w = w;
  return 0;
}

template <class C, class F, int P>
void bases_batch_launch_free(const void* d_pts, const void* d_scalars, int mont, const uint32_t* d_index, const MsmBatchChunk* d_chunks,
                             uint32_t n_chunks, void* d_partials, hipStream_t st) {
  if constexpr (std::is_same<F, FpField<C>>::value)
    k_msm_batch_chunk_bases<C, P><<<dim3((n_chunks + 63) / 64), dim3(64), 0, st>>>(
        (const Affine<FpField<C>>*)d_pts, (const uint32_t*)d_scalars, mont, d_index, d_chunks, n_chunks,
        (XYZZ<FpField<C>>*)d_partials);
  else
    k_msm_batch_chunk_bases_lp<C, P><<<dim3((unsigned)((2 * (size_t)n_chunks + 63) / 64)), dim3(64), 0, st>>>(
        (const Affine<Fp2Field<C>>*)d_pts, (const uint32_t*)d_scalars, mont, d_index, d_chunks, n_chunks,
        (XYZZ<Fp2Field<C>>*)d_partials);
}

// mlhip_bases_msm_batch_device behind its checks (api_bases.hip): k >= 1 checked offsets, base_index (host, may be null) within the
// handle's n_bases points, need = 1 + the largest base a pair reads (0: no pair)
template <class C, class F>
int bases_batch_device(mlhip_bases_batch_tables* t, const void* d_pts, size_t n_bases, const void* d_scalars, int mont,
                       const uint32_t* base_index, const uint64_t* offsets, size_t k, size_t need, void* d_out, hipStream_t st) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  (void)n_bases;
  const int w = bases_batch_window<C, F>();
  const size_t per = bases_batch_entries(w);
  const size_t row = kG1 ? sizeof(Affine28<C>) : sizeof(AffineG2_28<C>);
  const bool tabled = need > 0 && need * per * row <= bases_batch_cap_bytes();
  if (tabled && (t->w != w || t->n_tabled < need)) {
    int rc = bases_batch_grow<C, F>(t, d_pts, need, w, st);
    if (rc) return rc;
  }
  const size_t index_bytes = base_index ? (size_t)offsets[k] * 4 : 0;
  if (!tabled) {
    // mlhip_msm_batch's kernels over the handle's points: Straus chunks, and the bucket route for the long segments.  The
    // extra upload is [the index list | the slice rows].
    const int P = msm_batch_chunk_len<C, F>();
    MsmBucketCall<C, F> call;
    if (!call.plan(offsets, k, P)) return mlhip_rt::fail(MLHIP_EINVAL, "bases msm batch: more than 2^32 - 1 chunks");
    std::vector<uint32_t> extra;
    const void* up = base_index;
    if (!call.slices.empty()) {
      if (base_index) extra.assign(base_index, base_index + offsets[k]);
      extra.insert(extra.end(), call.slices.begin(), call.slices.end());
      up = extra.data();
    }
    return msm_batch_run<C, F>(
        call.L, up, index_bytes + call.slices.size() * sizeof(uint32_t), d_out, st,
        [&](const MsmBatchChunk* d_chunks, uint32_t n_chunks, const void* d_extra, void* part, void* d_scratch) {
          const uint32_t* d_index = base_index ? (const uint32_t*)d_extra : nullptr;
          if (n_chunks > call.slices.size()) {
            switch (P) {
              case 1: bases_batch_launch_free<C, F, 1>(d_pts, d_scalars, mont, d_index, d_chunks, n_chunks, part, st); break;
              case 2: bases_batch_launch_free<C, F, 2>(d_pts, d_scalars, mont, d_index, d_chunks, n_chunks, part, st); break;
              case 4: bases_batch_launch_free<C, F, 4>(d_pts, d_scalars, mont, d_index, d_chunks, n_chunks, part, st); break;
              default: bases_batch_launch_free<C, F, 8>(d_pts, d_scalars, mont, d_index, d_chunks, n_chunks, part, st); break;
            }
          }
          if (!call.slices.empty())
            call.launch(d_pts, MsmBucketIndexed{d_index}, d_scalars, mont, d_chunks,
                        (const uint32_t*)((const char*)d_extra + index_bytes), part, d_scratch, st);
        },
        call.scratch);
  }
  const int P = bases_batch_chunk_len<C, F>(offsets, k);
  MsmBatchLayout L;
  if (!msm_batch_layout(L, offsets, k, P)) return mlhip_rt::fail(MLHIP_EINVAL, "bases msm batch: more than 2^32 - 1 chunks");
  return msm_batch_run<C, F>(L, base_index, index_bytes, d_out, st,
                             [&](const MsmBatchChunk* d_chunks, uint32_t n_chunks, const void* d_extra, void* part, void*) {
    const uint32_t* d_index = base_index ? (const uint32_t*)d_extra : nullptr;
    if constexpr (kG1)
      k_bases_batch_chunk<C><<<dim3((n_chunks + 63) / 64), dim3(64), 0, st>>>(
          (const Affine28<C>*)t->buf, per, w, (const uint32_t*)d_scalars, mont, d_index, d_chunks, n_chunks, (XYZZ<F>*)part);
    else
      k_bases_batch_chunk_lp<C><<<dim3((unsigned)((2 * (size_t)n_chunks + 63) / 64)), dim3(64), 0, st>>>(
          (const AffineG2_28<C>*)t->buf, per, w, (const uint32_t*)d_scalars, mont, d_index, d_chunks, n_chunks, (XYZZ<F>*)part);
  });
}
#endif  // __HIPCC__

}  // namespace mlhip
