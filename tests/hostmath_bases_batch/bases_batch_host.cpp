// tests/hostmath_bases_batch -- g++ build (-DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) of the per-lane body
// of the batched MSM over resident bases (mathlib_amd/csrc/msm_bases_batch.h), replayed on the CPU in the order the kernels
// run it: the per-base tables T_b[j][m - 1] = [m 2^(wj)] B_b computed here by doublings and additions (entries whose
// multiplier does not fit 256 bits are the point at infinity, as k_fb_scalars makes them), converted to the carry-free rows
// the kernels read, then msm_batch_layout, bases_batch_chunk per chunk, the sum passes of msm_batch.h and xyzz_to_affine.
// G2 runs the lane-pair body over PairHost (both components in one host "lane pair").  Driven by
// tests/test_bases_batch_host.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_bases_batch.h"

using namespace mlhip;

// [m 2^(wj)] B for every (j, m) of one base, in the boundary form (the product kernels' tables before conversion)
template <class F>
static void host_table(std::vector<Affine<F>>& out, const Affine<F>& base, int w) {
  const int nw = fb_windows(w), row = 1 << (w - 1);
  out.assign((size_t)nw * row, Affine<F>());
  XYZZ<F> pj;  // [2^(wj)] B
  xyzz_from_affine<F>(pj, base);
  for (int j = 0; j < nw; j++) {
    XYZZ<F> acc;
    xyzz_set_inf<F>(acc);
    for (int m = 1; m <= row; m++) {
      xyzz_add<F>(acc, pj);
      const int top = j * w + 31 - __builtin_clz((unsigned)m);  // highest set bit of m 2^(wj)
      if (top >= 256) {
        F::zero(out[(size_t)j * row + m - 1].x);
        F::zero(out[(size_t)j * row + m - 1].y);
      } else {
        xyzz_to_affine<F>(out[(size_t)j * row + m - 1], acc);
      }
    }
    for (int d = 0; d < w; d++) {
      XYZZ<F> t;
      xyzz_dbl<F>(t, pj);
      pj = t;
    }
  }
}

template <class C>
static void to_row(Affine28<C>& r, const Affine<FpField<C>>& p) {
  affine28_from<C>(r, p);
}
template <class C>
static void to_row(Affine28L<typename PairHost<C>::V>& r, const Affine<Fp2Field<C>>& p) {
  fp28_from_fp<C>(r.x.v[0], p.x.c0);
  fp28_from_fp<C>(r.x.v[1], p.x.c1);
  fp28_from_fp<C>(r.y.v[0], p.y.c0);
  fp28_from_fp<C>(r.y.v[1], p.y.c1);
}
template <class C>
static void from_acc(XYZZ<FpField<C>>& r, const XYZZ28<C>& a, bool inf) {
  xyzz28_to<C>(r, a, inf);
}
template <class C>
static void from_acc(XYZZ<Fp2Field<C>>& r, const XYZZ28L<typename PairHost<C>::V>& a, bool inf) {
  if (inf) {
    xyzz_set_inf<Fp2Field<C>>(r);
    return;
  }
  fp28_to_fp<C>(r.x.c0, a.x.v[0]);
  fp28_to_fp<C>(r.x.c1, a.x.v[1]);
  fp28_to_fp<C>(r.y.c0, a.y.v[0]);
  fp28_to_fp<C>(r.y.c1, a.y.v[1]);
  fp28_to_fp<C>(r.zz.c0, a.zz.v[0]);
  fp28_to_fp<C>(r.zz.c1, a.zz.v[1]);
  fp28_to_fp<C>(r.zzz.c0, a.zzz.v[0]);
  fp28_to_fp<C>(r.zzz.c1, a.zzz.v[1]);
}

template <class C, class F, class Ops>
static int batch(int w, int P, const void* bases, size_t n_bases, const void* scalars, int mont, const uint32_t* index,
                 const uint64_t* offsets, size_t k, void* out, uint64_t* stats) {
  typedef typename Ops::Row Row;
  const size_t per = bases_batch_entries(w);
  std::vector<Row> tab(n_bases * per);
  std::vector<Affine<F>> t;
  for (size_t b = 0; b < n_bases; b++) {
    host_table<F>(t, ((const Affine<F>*)bases)[b], w);
    for (size_t e = 0; e < per; e++) to_row<C>(tab[b * per + e], t[e]);
  }
  MsmBatchLayout L;
  if (!msm_batch_layout(L, offsets, k, P)) return -1;
  const uint32_t* sc = (const uint32_t*)scalars;
  std::vector<XYZZ<F>> cur(L.chunks.size()), next;
  uint64_t bad = 0;
  for (size_t c = 0; c < L.chunks.size(); c++) {
    const MsmBatchChunk ch = L.chunks[c];
    if (ch.count < 1 || ch.count > (uint32_t)P) return -2;
    typename Ops::Acc acc;
    bool inf;
    bases_batch_chunk<Ops>(acc, inf, sc + 8 * ch.first, index ? index + ch.first : nullptr, ch.base0, ch.count, mont != 0, w,
                           [&](Row& q, uint32_t b, uint32_t e) {
                             if (b >= n_bases || e >= per) {
                               bad++;
                               b = 0;
                               e = 0;
                             }
                             q = tab[(size_t)b * per + e];
                           });
    from_acc<C>(cur[c], acc, inf);
  }
  if (bad) return -7;  // a row outside the tables
  const size_t passes = L.pass_begin.size() - 1;
  for (size_t q = 0; q < passes; q++) {
    const size_t g0 = L.pass_begin[q], g1 = L.pass_begin[q + 1];
    next.assign(g1 - g0, XYZZ<F>());
    for (size_t g = g0; g < g1; g++) {
      const MsmBatchGroup gr = L.groups[g];
      if ((size_t)gr.begin + gr.count > cur.size()) return -4;
      msm_batch_sum<F, MsmBatchOps<F>>(next[g - g0], gr.count, [&](XYZZ<F>& p, uint32_t i) { p = cur[gr.begin + i]; });
    }
    cur.swap(next);
  }
  if (cur.size() != k) return -3;
  Affine<F>* o = (Affine<F>*)out;
  for (size_t s = 0; s < k; s++) xyzz_to_affine<F>(o[s], cur[s]);
  if (stats) {
    stats[0] = L.chunks.size();
    stats[1] = passes;
  }
  return 0;
}

template <class C>
static int batch_group(int group, int w, int P, const void* bases, size_t n_bases, const void* scalars, int mont,
                       const uint32_t* index, const uint64_t* offsets, size_t k, void* out, uint64_t* stats) {
  if (group == 1) return batch<C, FpField<C>, BasesBatchOpsG1<C>>(w, P, bases, n_bases, scalars, mont, index, offsets, k, out, stats);
  return batch<C, Fp2Field<C>, BasesBatchOpsLp<C, PairHost<C>>>(w, P, bases, n_bases, scalars, mont, index, offsets, k, out, stats);
}

extern "C" {
// out[s] = the affine sum of segment s over the n_bases bases (index: one base per pair, or null: pair j of a segment takes
// base j); stats = {chunks, passes} (may be null).  0 on success.
int hbb_bases_batch(int curve, int group, int w, int P, const void* bases, size_t n_bases, const void* scalars, int mont,
                    const uint32_t* index, const uint64_t* offsets, size_t k, void* out, uint64_t* stats) {
  if (w < BASES_BATCH_W_MIN || w > BASES_BATCH_W_MAX || !bases_batch_p_valid(P)) return -5;
  switch (curve) {
    case 0: return batch_group<Bn254>(group, w, P, bases, n_bases, scalars, mont, index, offsets, k, out, stats);
    case 1: return batch_group<Bls381>(group, w, P, bases, n_bases, scalars, mont, index, offsets, k, out, stats);
    case 2: return batch_group<Bls377>(group, w, P, bases, n_bases, scalars, mont, index, offsets, k, out, stats);
    default: return -6;
  }
}
}
